#!/usr/bin/env python3
"""A voxel subsample of every scene cloud (one point per cell of subsample_voxel metres) and the kept indices, on an MI355X:
--config <yaml> [--scene <id> ...]; the work is done by beyond_fixed_forms_amd."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beyond_fixed_forms_amd.cli import subsample_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(subsample_main())
