#!/usr/bin/env python
"""Drop-in for the reference's windowStats.py: per window and column of a table of per-site numbers, mean / median / min / max / sd /
sum / quantiles as NumPy computes them, on an MI355X by libpopgen_hip.so (k_ws_stats).  See genomics_general_amd/wstats.py."""
import sys

from genomics_general_amd.cli import windowstats_main

if __name__ == "__main__":
    sys.exit(windowstats_main())
