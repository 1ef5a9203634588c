#!/usr/bin/env python3
"""A class's 3-D instances clustered by density, DBSCAN with a deterministic border rule (the stage's own file format),
on an MI355X: --config <yaml> --cls "<class>" [--stage final|mask_3d]; the work is done by beyond_fixed_forms_amd."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beyond_fixed_forms_amd.cli import cluster_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(cluster_main())
