#!/usr/bin/env python
"""Drop-in for the reference's tools/genoToPlink.py: a `.geno` file as PLINK .ped / .map (and .fam) files; the cells expanded into
alleles and transposed into sample rows on an MI355X by libpopgen_hip.so (k_ped_lines, k_ped_map, k_ped_tile).  See
genomics_general_amd/genoplink.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genomics_general_amd.cli import genotoplink_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(genotoplink_main())
