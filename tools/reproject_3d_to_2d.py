#!/usr/bin/env python3
"""A class's 3-D instances rendered back into the colour frames as 2-D masks (mask_2d file format), on an MI355X:
--config <yaml> --cls "<class>" [--stage final|mask_3d] [--every n]; the work is done by beyond_fixed_forms_amd."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beyond_fixed_forms_amd.cli import reproject_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(reproject_main())
