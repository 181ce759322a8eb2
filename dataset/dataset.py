"""Re-export of the on-GPU `SynDataset.snr_mix` (dataset/dataset.py:236-264) and `SynDataset.add_reverb` (:215-233), and of the
device-resident file-list dataset that stands for the class itself (cruse_amd.filepairs.DeviceFilePairs)."""
from cruse_amd.data import add_reverb as _add_reverb
from cruse_amd.filepairs import DeviceFilePairs  # noqa: F401
from cruse_amd.data import snr_mix  # noqa: F401


def add_reverb(cln_wav, rir_wav, channels=1, predelay=50, sr=16000):
    """The reference's call shape: cln_wav [L], rir_wav [R, 1] (or [R]) on the device -> (wav_tgt, wav_early_tgt), each [L, 1]
    (cruse_amd.data.add_reverb states the repairs)."""
    if rir_wav.dim() == 2:
        if rir_wav.shape[1] != 1:
            raise NotImplementedError("add_reverb: multi-channel responses are not built (SURVEY section 2)")
        rir_wav = rir_wav[:, 0]
    if cln_wav.dim() != 1:
        raise NotImplementedError("add_reverb: the reference's call takes one mono clip [L]; batches go through cruse_amd.data.add_reverb")
    full, early = _add_reverb(cln_wav, rir_wav, channels=channels, predelay=predelay, sr=sr)
    return full[:, None], early[:, None]


class SynDataset:
    """Only the mixing and reverberation steps of the reference class are on this path; they are staticmethods there (dataset.py:215, :235)."""
    snr_mix = staticmethod(snr_mix)
    add_reverb = staticmethod(add_reverb)
