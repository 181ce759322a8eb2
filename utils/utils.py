"""Re-export so the reference dotted paths utils.utils.PreProcess (utils/utils.py:365-455) and utils.utils.postfiltering /
envelope_postfiltering (:345-362) resolve."""
from cruse_amd.acoustics.preprocess import PreProcess  # noqa: F401
from cruse_amd.acoustics.postfilter import envelope_postfiltering, postfiltering  # noqa: F401
