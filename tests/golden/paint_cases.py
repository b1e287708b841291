"""distPaint.py goldens: fixtures, side files and command lines (tests/golden/make_golden_paint.py runs the unmodified reference on
them; tests/test_paint_cpu.py and tests/test_gpu_paint.py compare byte for byte).

{geno}: the case's fixture, {dir}: tests/golden.  The output file is appended as `-o`; a case with gz=True writes `-o *.gz` and the
golden holds the gunzipped text."""

# haploid fixtures written by make_golden_paint.py (the `haplo` fixture of cases.py is used as it is).  groups: (name prefix, number of
# individuals, source population or None = a mosaic that changes source every `block` positions); names: the header order, None = as
# generated (which is sorted order)
PAINT_FIXTURES = {
    # 24 individuals, 30 % missing calls: windows of ~100 sites in which pairs share ~49 called sites
    "paint_mosaic": dict(seed=20261018, groups=[("a", 9, 0), ("b", 2, 1), ("c", 1, 2), ("d", 4, 3), ("q", 8, None)], n_src=4,
                         scaf_len=[2000, 1500], step=5, miss=0.30, block=400, names=None),
    # 16 individuals under a header that is NOT in sorted order: the alignment's rows are sorted by name, distPaint.py indexes them by column
    "paint_unsorted": dict(seed=20261019, groups=[("x", 4, 0), ("m", 4, 1), ("e", 3, 2), ("t", 5, None)], n_src=3,
                           scaf_len=[1800], step=6, miss=0.05, block=300,
                           names=["t3", "x0", "m2", "e1", "t0", "x3", "m0", "t4", "e0", "x1", "m3", "t1", "e2", "x2", "m1", "t2"]),
}

PAINT_AUX_FILES = {
    # an individual the file does not have (skipped), a population no -p names (skipped), members of a and b
    "paint_pops.txt": "a0 A\na3 A\nzz9 A\nb0 B\nb1 B\nd0 D\na5 A\nd1 Z\n",
    "paint_coords.txt": "chr1 1 400 first\nchr1 401 402 empty\nchr2 100 900 third\nchr1 1500 2000 fourth\n",
    "paint_include.txt": "chr1\n",
}

A9 = "a0,a1,a2,a3,a4,a5,a6,a7,a8"
FOUR = ["-p", "A", A9, "-p", "B", "b0,b1", "-p", "C", "c0", "-p", "D", "d0,d1,d2,d3"]
THREE = ["-p", "A", A9, "-p", "B", "b0,b1", "-p", "D", "d0,d1,d2,d3"]
HAPLO = ["-p", "one", "s0_A,s0_B,s1_A", "-p", "two", "s3_A,s3_B,s4_A,s4_B"]
UNSORTED = ["-p", "X", "x0,x1,x2,x3", "-p", "M", "m0,m1,m2,m3", "-p", "E", "e0,e1,e2"]

PAINT_CASES = [
    dict(name="haplo_test", fixture="haplo", argv=["-g", "{geno}", "-w", "1000", "-m", "20"] + HAPLO),
    dict(name="haplo_delta", fixture="haplo", argv=["-g", "{geno}", "-w", "1000", "-m", "20", "--delta_threshold", "0.002"] + HAPLO),
    dict(name="haplo_gz_out", fixture="haplo", gz=True, argv=["-g", "{geno}", "-w", "500", "-s", "250", "-m", "20", "-T", "2"] + HAPLO),
    dict(name="unsorted_test", fixture="paint_unsorted", argv=["-g", "{geno}", "-w", "600", "-m", "30", "--p_threshold", "0.2"] + UNSORTED),
    dict(name="unsorted_delta0", fixture="paint_unsorted", argv=["-g", "{geno}", "-w", "600", "-m", "30", "--delta_threshold", "0"] + UNSORTED),
    # reference populations of 9, 2, 1 and 4 individuals.  Against a population of ONE no rank sum reaches p <= 0.05 (9 against 1: 0.058 at best,
    # 4 against 1: 0.079), so the cases with all four populations carry a --p_threshold under which individuals are assigned
    dict(name="mosaic_four_pops", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "500", "-m", "10", "--p_threshold", "0.1"] + FOUR),
    dict(name="mosaic_three_pops_dup", fixture="paint_mosaic",
         argv=["-g", "{geno}", "-w", "500", "-m", "10", "-p", "A", "a0,a1,a1,a2", "-p", "B", "b0,b1,b0", "-p", "D", "d0,d1,d2,d3"]),
    dict(name="mosaic_popsfile", fixture="paint_mosaic",
         argv=["-g", "{geno}", "-w", "500", "-m", "10", "-p", "A", "a8", "-p", "B", "-p", "D", "d3,d2", "--popsFile", "{dir}/paint_pops.txt"]),
    # -m close to the windows' ~100 sites and the pairs' ~49 shared calls: nan pairs, all-nan populations, nan in the best population
    dict(name="mosaic_nan_test", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "500", "-m", "50"] + FOUR),
    dict(name="mosaic_nan_test_three", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "500", "-m", "48", "--p_threshold", "0.2"] + THREE),
    dict(name="mosaic_nan_delta", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "500", "-m", "50", "--delta_threshold", "0.02"] + FOUR),
    dict(name="mosaic_nan_delta_three", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "500", "-m", "47", "--delta_threshold", "0.01"] + THREE),
    dict(name="mosaic_sites_windows", fixture="paint_mosaic",
         argv=["-g", "{geno}", "--windType", "sites", "-w", "80", "-O", "20", "-D", "600", "-m", "30", "--p_threshold", "0.1"] + FOUR),
    # (-m 0 = the window size: with missing calls no pair shares that many sites, every mean is nan and np.argmin answers 0 throughout)
    dict(name="mosaic_sites_m0", fixture="paint_mosaic", argv=["-g", "{geno}", "--windType", "sites", "-w", "60", "-m", "0"] + THREE),
    dict(name="mosaic_predefined", fixture="paint_mosaic",
         argv=["-g", "{geno}", "--windType", "predefined", "--windCoords", "{dir}/paint_coords.txt", "-m", "5", "--p_threshold", "0.1"] + FOUR),
    dict(name="mosaic_predefined_id_failed", fixture="paint_mosaic",
         argv=["-g", "{geno}", "--windType", "predefined", "--windCoords", "{dir}/paint_coords.txt", "-m", "5", "--addWindowID",
               "--writeFailedWindows"] + THREE),
    dict(name="mosaic_id_failed", fixture="paint_mosaic",
         argv=["-g", "{geno}", "-w", "700", "-s", "700", "-m", "62", "--addWindowID", "--writeFailedWindows", "--delta_threshold", "0.05"] + THREE),
    dict(name="mosaic_noresult9", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "500", "-m", "10", "--noresult", "9", "--p_threshold", "0.2"] + FOUR),
    dict(name="mosaic_p001", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "250", "-m", "10", "--p_threshold", "0.01", "--minData", "0.5",
                                                           "--samples", "q0,q1", "-p", "A", A9, "-p", "D", "d0,d1,d2,d3"]),
    dict(name="mosaic_include", fixture="paint_mosaic", argv=["-g", "{geno}", "-w", "500", "-m", "10", "--include", "{dir}/paint_include.txt", "--p_threshold", "0.15"] + FOUR),
]
