"""WAV reading for the file-list dataset (filepairs.DeviceFilePairs): 16-bit PCM through the standard library's `wave`, nothing else.
The reference reads with librosa (dataset/dataset.py:155), which decodes anything; here every other encoding is refused by name."""
from __future__ import annotations

import os
import wave
from typing import List, Tuple

import numpy as np


def read_pcm16(path: str) -> Tuple[np.ndarray, int, int]:
    """-> (int16 [frames * channels] interleaved, channels, rate).  Anything but uncompressed 16-bit PCM in a RIFF/WAVE container
    raises a ValueError that names the file and what was found."""
    try:
        with wave.open(path, "rb") as w:
            channels, width, rate, frames, comp = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.getcomptype()
            if comp != "NONE" or width != 2:
                raise ValueError(f"{path}: {8 * width}-bit samples, compression {comp!r}; only uncompressed 16-bit PCM is read")
            if channels < 1 or rate < 1:
                raise ValueError(f"{path}: {channels} channels at {rate} Hz")
            raw = w.readframes(frames)
    except (wave.Error, EOFError) as ex:                      # not RIFF, not WAVE, a format tag `wave` does not decode, a cut header
        raise ValueError(f"{path}: not a PCM WAV file ({ex or type(ex).__name__})") from ex
    pcm = np.frombuffer(raw, dtype="<i2").astype(np.int16, copy=False)
    pcm = pcm[:pcm.shape[0] // channels * channels]           # a cut last frame is dropped
    if pcm.shape[0] == 0:
        raise ValueError(f"{path}: no samples")
    return pcm, channels, rate


def offset_and_limit(dataset_list: List[str], offset, limit) -> List[str]:
    """BaseDataset._offset_and_limit (dataset/dataset.py:27-32)"""
    dataset_list = dataset_list[offset:]
    if limit:
        dataset_list = dataset_list[:limit]
    return dataset_list


def read_list(list_file: str, offset=0, limit=None) -> List[str]:
    """One path per line (dataset/dataset.py:80-83: the line ends are stripped, `~` in the list's own name is expanded), then
    _offset_and_limit.  Empty lines are dropped and `~` is expanded in the entries too."""
    with open(os.path.abspath(os.path.expanduser(list_file)), "r") as f:
        lines = [line.rstrip("\n") for line in f]
    lines = [os.path.expanduser(line) for line in lines if line.strip()]
    return offset_and_limit(lines, offset or 0, limit)
