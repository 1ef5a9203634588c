#!/usr/bin/env python3
"""A scene's prediction assembled from all of its query classes, duplicates removed by a 3-D mask NMS, on an MI355X:
--config <yaml> (--cls a --cls b ... | --all-classes) [--stage final|mask_3d] [--point-labels]; the work is done by
beyond_fixed_forms_amd."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beyond_fixed_forms_amd.cli import assemble_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(assemble_main())
