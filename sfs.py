#!/usr/bin/env python
"""Drop-in for the reference's sfs.py: 1-D to 4-D site-frequency spectra from genotypes or freq.py tables, counted on an MI355X by
libpopgen_hip.so (k_sfs_rows / k_sfs_base / k_sfs_target).  See genomics_general_amd/sfs.py."""
import sys

from genomics_general_amd.cli import sfs_main

if __name__ == "__main__":
    sys.exit(sfs_main())
