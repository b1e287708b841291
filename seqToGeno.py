#!/usr/bin/env python
"""Drop-in for the reference's seqToGeno.py: a fasta or phylip alignment as `.geno` sites; the byte transpose from sequences back to
site-major text on an MI355X by libpopgen_hip.so (k_s2g_lines, k_s2g_gather, k_s2g_tile).  See genomics_general_amd/seqgeno.py."""
import sys

from genomics_general_amd.cli import seqtogeno_main

if __name__ == "__main__":
    sys.exit(seqtogeno_main())
