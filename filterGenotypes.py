#!/usr/bin/env python
"""Drop-in for the reference's filterGenotypes.py: `.geno` sites filtered (siteTest, include / exclude, thinning per pod) on an MI355X
by libpopgen_hip.so (k_filt_lines, k_filt_thin), host threads for irregular text.  See genomics_general_amd/filtergeno.py."""
import sys

from genomics_general_amd.filtergeno import filter_main

if __name__ == "__main__":
    sys.exit(filter_main())
