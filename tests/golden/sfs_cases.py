"""Golden cases of the sfs.py drop-in, shared by make_golden_sfs.py (runs the UNMODIFIED reference) and tests/test_gpu_sfs.py.

A case: name, argv in the reference's syntax with {geno} (the case's `.geno.gz` fixture of cases.py), {dir} (tests/golden) and {out} (the
case's output directory) placeholders; `pipe`: everything goes to stdout (kept as `stdout`); `fails`: the reference exits non-zero and
writes nothing.  The table inputs are goldens of the reference's own freq.py (cases.py: abba_freq_counts, abba_freq_derived_counts_keepnan).
Outputs live in tests/golden/sfs/<name>/."""
from cases import pops_args

P2, P3, P4, B4 = pops_args(8, 2), pops_args(12, 3), pops_args(16, 4), pops_args(8, 4)

SFS_AUX_FILES = {
    # overlapping regions across 2^31, a single position (start only), a region on the second scaffold, one no site falls in
    "bigpos_regions.txt": "chr1 2147483000 2147484000\nchr1 2147483600 2147485000 extra\nchr1 2147483650\nchr2 3000000100 3000000900\nchr2 5 9\n",
}

SFS_CASES = [
    dict(name="c1_1d", fixture="c1", argv=["-i", "{geno}", "--inputType", "genotypes", "--pref", "{out}/"] + P2),
    dict(name="c1_pairs_pipe", fixture="c1", pipe=True, argv=["-i", "{geno}", "--inputType", "genotypes", "--doPairs", "--pipe"] + P2),
    dict(name="c1_all", fixture="c1", argv=["-i", "{geno}", "--inputType", "genotypes", "--pref", "{out}/"]),
    dict(name="abba_trios_quartets", fixture="abba",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--doTrios", "--doQuartets", "--pref", "{out}/"] + P4),
    dict(name="abba_polarized_pairs", fixture="abba",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--polarized", "--doPairs", "--pref", "{out}/"] + P4),
    dict(name="abba_outgroup_not_last", fixture="abba",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--outgroup", "pop1", "--doPairs", "--doTrios", "--pref", "{out}/pre_", "--suff", ".txt"] + P4),
    dict(name="abba_fspops_popsfile", fixture="abba",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--popsFile", "{dir}/abba_pops.txt", "--FSpops", "pop0", "pop2", "--FSpops", "pop3",
               "--FSpops", "pop1", "pop2", "pop3", "pop0", "--pref", "{out}/"]),
    dict(name="abba_pairs_alleles", fixture="abba_pairs",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--genoFormat", "alleles", "--doPairs", "--pref", "{out}/"] + P4),
    dict(name="abba_diplo_polarized", fixture="abba_diplo",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--genoFormat", "diplo", "--polarized", "--pref", "{out}/"] + P4),
    dict(name="sparse_pairs_trios", fixture="sparse",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--doPairs", "--doTrios", "--pref", "{out}/"] + P3),
    dict(name="holes_pairs", fixture="holes", argv=["-i", "{geno}", "--inputType", "genotypes", "--doPairs", "--pref", "{out}/"] + pops_args(6, 2)),
    dict(name="multi_pairs_polarized", fixture="multi",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--doPairs", "--polarized", "--pref", "{out}/"] + pops_args(9, 3)),
    dict(name="mixed_ploidyfile", fixture="mixed",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--ploidyFile", "{dir}/mixed_ploidy.txt", "--doPairs", "--pref", "{out}/"] + pops_args(10, 2)),
    dict(name="bigpos_regions_overlap", fixture="bigpos",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--doPairs", "--polarized", "--regions", "chr1:2147483000-2147484000",
               "chr1:2147483600-2147485000", "chr2:3000000900-3000000100", "--pref", "{out}/"] + B4),
    dict(name="bigpos_regionsfile_include", fixture="bigpos",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--regionsFile", "{dir}/bigpos_regions.txt", "--include", "chr1", "--pref", "{out}/"] + B4),
    dict(name="bigpos_exclude", fixture="bigpos",
         argv=["-i", "{geno}", "--inputType", "genotypes", "--exclude", "chr1", "chrX", "--doPairs", "--pref", "{out}/"] + B4),
    dict(name="bigpos_region_without_coordinates", fixture="bigpos", fails=True,
         argv=["-i", "{geno}", "--inputType", "genotypes", "--regions", "chr1", "--pref", "{out}/"] + B4),
    # ---- table inputs: the reference's freq.py wrote them ----
    dict(name="table_base_polarized", fixture=None,
         argv=["-i", "{dir}/abba_freq_counts.out", "--inputType", "baseCounts", "--polarized", "--doPairs", "--pref", "{out}/"]),
    dict(name="table_base_minor_regions", fixture=None,
         argv=["-i", "{dir}/abba_freq_counts.out", "--inputType", "baseCounts", "-p", "pop2", "-p", "pop0", "--doPairs", "--regions", "chr1:1-3000",
               "chr2:100-2000", "chr1:2500-9000", "--pref", "{out}/"]),
    dict(name="table_target", fixture=None,
         argv=["-i", "{dir}/abba_freq_derived_counts_keepnan.out", "-p", "pop0", "-p", "pop1", "-p", "pop2", "--doPairs", "--doTrios", "--pref", "{out}/"]),
]
