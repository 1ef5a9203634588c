#!/usr/bin/env python3
"""The frames that see each 3-D instance best and the boxes to crop it with, on an MI355X:
--config <yaml> --cls "<class>" [--stage final|mask_3d] [--every n] [--assembled]; the work is done by
beyond_fixed_forms_amd."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beyond_fixed_forms_amd.cli import select_views_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(select_views_main())
