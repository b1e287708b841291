#!/usr/bin/env python
"""Drop-in for the reference's genoToSeq.py: a `.geno` file, or every window or contig of it, as fasta / phylip alignments; the byte
transpose from site-major text to sequences on an MI355X by libpopgen_hip.so (k_seq_lines, k_seq_tile).  See
genomics_general_amd/genoseq.py."""
import sys

from genomics_general_amd.cli import genotoseq_main

if __name__ == "__main__":
    sys.exit(genotoseq_main())
