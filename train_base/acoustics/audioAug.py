"""Re-export so the reference dotted path train_base.acoustics.audioAug resolves."""
from cruse_amd.acoustics.audio_aug import *  # noqa: F401,F403
from cruse_amd.acoustics.audio_aug import (REGISTERED_SecFilter, REGISTERED_SecFilter_freq, compositeSecFilt, draw_hp_filters,  # noqa: F401
                                           draw_sec_filters, high_pass, high_shelf, hp_filter, low_pass, low_shelf, notch, peaking_eq)
