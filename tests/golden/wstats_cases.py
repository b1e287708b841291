"""The windowStats.py golden cases (tests/golden/make_golden_wstats.py writes the fixtures and records the outputs with the unmodified
reference under the `np.NaN = np.nan` shim): (name, fixture, argv, through stdin).  @G stands for tests/golden.  Fixtures, under wstats/:
  main.tsv         two scaffolds, three columns a b c: decimals, integers, exponents, nan cells; a gap wider than a window (an empty
                   coordinate window), windows of one site
  quirks.tsv       `1e3`, `07`, `inf`, `-inf`; the irregular spellings NumPy's cast takes (`1_0`, `1.`, `.5` are regular or not as
                   pg_ws_core.h says; `1e400`, `infinity`, `-nan`, `+nan`, 16 and 17 digits, `1e23`, `1e-23`, `1e-400`); a '#' line; runs
                   of blanks and tabs between the fields; scaffold c1 comes back behind c2
  bad.tsv          a cell that is no number (`x`) in a window that -m fails: the reference never converts it
  allnan.tsv       a column without a value in a window that has enough sites
  header_only.tsv  no site: a run without any window
  headerless.tsv   main.tsv without its first line (--headers, through stdin)
  dup.tsv          a header that holds the name `a` twice
  coords.txt       a --windCoords file: windows in the file's order, one without sites, one of a scaffold the table lacks
Recorded with NumPy NUMPY_VERSION; the statistics are NumPy's to the last bit, so tests that compare against NumPy itself skip under
another version (the goldens hold under any)."""
import gzip
import os

HERE = os.path.dirname(os.path.abspath(__file__))
NUMPY_VERSION = "2.2.6"

ALL = ["mean", "median", "min", "max", "sd", "sum", "q5", "q10", "q25", "q75", "q90", "q95"]

CASES = [
    ("coord_default", "main", ["-w", "100"], False),
    ("coord_explicit", "main", ["--windType", "coordinate", "-w", "150"], False),
    ("coord_step", "main", ["-w", "100", "-s", "40"], False),
    ("coord_min5", "main", ["-w", "100", "-m", "5"], False),
    ("coord_m0", "main", ["-w", "12", "-m", "0"], False),
    ("coord_failed_flag", "main", ["-w", "100", "-m", "5", "--writeFailedWindows"], False),
    ("sites_10", "main", ["--windType", "sites", "-w", "10"], False),
    ("sites_overlap", "main", ["--windType", "sites", "-w", "10", "-O", "4"], False),
    ("sites_maxdist", "main", ["--windType", "sites", "-w", "10", "-D", "60", "-m", "3"], False),
    ("predefined", "main", ["--windType", "predefined", "--windCoords", "@G/wstats/coords.txt"], False),
    ("columns_order", "main", ["-w", "100", "--columns", "c", "a"], False),
    ("columns_one", "main", ["-w", "300", "--columns", "b", "--stats", "median", "q75"], False),
    ("headers_stdin", "headerless", ["-w", "100", "--headers", "scaffold", "position", "x", "y", "z"], True),
    ("stdin_plain", "main", ["--windType", "sites", "-w", "25", "-m", "5"], True),
] + [("stat_" + s, "main", ["-w", "200", "--stats", s], False) for s in ALL] + [
    ("stats_all", "main", ["-w", "100", "--stats"] + ALL, False),
    ("stats_repeated", "main", ["-w", "100", "--stats", "mean", "mean", "q5", "mean", "max"], False),
    ("quirks_all", "quirks", ["-w", "50", "--stats"] + ALL, False),
    ("quirks_sites", "quirks", ["--windType", "sites", "-w", "7", "-O", "2", "-m", "2", "--stats"] + ALL, False),
    ("bad_in_failed_window", "bad", ["-w", "100", "-m", "4"], False),
    ("allnan_column", "allnan", ["-w", "100", "--stats", "mean", "median", "sd", "sum", "q25"], False),
    ("no_window", "header_only", ["-w", "100"], False),
    ("dup_names", "dup", ["-w", "100", "--stats", "mean", "sum"], False),
    ("dup_names_column", "dup", ["-w", "100", "--columns", "a", "b", "--stats", "mean", "sum"], False),
]

# the cases in which no window has enough sites: nothing is computed, on the device or on host threads
NOTHING = {"coord_m0", "no_window"}
# ... those with cells of a spelling the parser hands to float() (the irregular spellings; a cell that is no number at all)
HOST_BLOCKS = {"quirks_all", "quirks_sites", "bad_in_failed_window"}
# ... and those whose statistics the device computes from cells of the regular spelling alone
DEVICE = [name for name, _, _, _ in CASES if name not in NOTHING and name not in HOST_BLOCKS]


def fixture_path(name):
    return os.path.join(HERE, "wstats", name + ".tsv")


def golden(name):
    with gzip.open(os.path.join(HERE, "wstats", name + ".out.gz"), "rb") as f:
        return f.read()
