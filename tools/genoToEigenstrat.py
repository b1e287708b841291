#!/usr/bin/env python
"""Drop-in for the reference's tools/genoToEigenstrat.py: the biallelic sites of a `.geno` file written as EIGENSTRAT .geno / .snp /
.ind files on an MI355X by libpopgen_hip.so (k_eig_lines) instead of a GenomeSite per line.  See genomics_general_amd/genoeig.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genomics_general_amd.genoeig import genoeig_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(genoeig_main())
