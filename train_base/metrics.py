"""train_base/metrics.py of the reference on the HIP path: SI_SDR, STOI and SDR on the device (cruse_amd/metrics.py); PESQ is not built."""
from cruse_amd.metrics import ESTOI, EXTENSION_METRICS, REGISTERED_METRICS, SI_SDR, STOI, estoi, si_sdr, stoi  # noqa: F401
from cruse_amd.metrics import SDR, UNREGISTERED_REFERENCE_METRICS, sdr  # noqa: F401
