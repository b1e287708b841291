#!/usr/bin/env python
"""Drop-in for the reference's distPaint.py: for every window and (haploid) individual, the reference population it is nearest to, by
a rank-sum test or a minimum gap between the two lowest mean distances; pair counts and decision on an MI355X by libpopgen_hip.so
(the pack and pair kernels, k_paint).  See genomics_general_amd/cli.py (distpaint_main)."""
import sys

from genomics_general_amd.cli import distpaint_main

if __name__ == "__main__":
    sys.exit(distpaint_main())
