#!/usr/bin/env python
"""Drop-in for the reference's mergeGeno.py: `.geno` files joined by site -- a sorted join of the files' lines on an MI355X by
libpopgen_hip.so (k_merge_keys, k_merge_lines / k_merge_pos, k_merge_emit) instead of a walk over every position of the genome.  See
genomics_general_amd/mergegeno.py."""
import sys

from genomics_general_amd.cli import mergegeno_main

if __name__ == "__main__":
    sys.exit(mergegeno_main())
