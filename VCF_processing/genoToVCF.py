#!/usr/bin/env python
"""Drop-in for the reference's VCF_processing/genoToVCF.py: `.geno` sites written as VCF rows on an MI355X by libpopgen_hip.so
(k_gvcf_lines) instead of a GenomeSite per line.  See genomics_general_amd/genovcf.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genomics_general_amd.genovcf import genovcf_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(genovcf_main())
