#!/usr/bin/env python3
"""Drop-in for the reference's evaluation/eval/eval_scannet200.py (its --cls, files and exit codes; the label
tables come from --label-table); the work is done by beyond_fixed_forms_amd on an MI355X."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beyond_fixed_forms_amd.cli import evaluation_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(evaluation_main())
