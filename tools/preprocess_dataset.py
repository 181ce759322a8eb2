"""Screen a WAV file list on the device and write the selected list (cruse_amd.screen; the reference's dataset/preprocess_dataset.py):

    python tools/preprocess_dataset.py (--list files.txt | --dir DIR) --out selected.txt [--rejected-prefix rejected] [--csv stats.csv]
        [--min-duration 3] [--clipping-threshold 0.999] [--min-activity 0.6] [--max-rt60 1.0] [--total-hrs 100] [--rt60]

Prints the reference's summary block: original files, selected hours and files, and the four rejection counts."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from cruse_amd.screen import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
