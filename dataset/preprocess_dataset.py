"""Re-export of the list builder at the reference's import path (dataset/preprocess_dataset.py): cruse_amd.screen.  Importing this module
runs nothing; `python -m dataset.preprocess_dataset --list files.txt --out selected.txt ...` is tools/preprocess_dataset.py."""
from cruse_amd.screen import decide, find_files, main, screen_files, summary, write_csv, write_lists  # noqa: F401
from cruse_amd.wavio import offset_and_limit  # noqa: F401

if __name__ == "__main__":
    import sys
    sys.exit(main())
