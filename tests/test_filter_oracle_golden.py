"""oracle/filter_oracle.py (a plain-Python restatement of filterGenotypes.py) pinned against the outputs of the UNMODIFIED reference:
all 37 goldens of tests/golden/filter byte for byte (-of randomAllele by membership), and the line of every case on which the
reference's worker raises (tests/test_filter_cpu.py's HANGS)."""
import gzip
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, ROOT)
from filter_cases import CASES, fixture_path  # noqa: E402

from oracle.filter_oracle import filter_reference  # noqa: E402
from test_filter_cpu import HANGS  # noqa: E402


def _text(fixture):
    p = fixture_path(fixture)
    with (gzip.open(p, "rb") if p.endswith(".gz") else open(p, "rb")) as f:
        return f.read()


def test_every_golden_is_covered():
    assert len(CASES) == 37
    assert sorted(f[:-7] for f in os.listdir(os.path.join(GOLD, "filter")) if f.endswith(".out.gz")) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("name,fixture,argv", CASES, ids=[c[0] for c in CASES])
def test_oracle_reproduces_the_reference(name, fixture, argv):
    res = filter_reference([a.replace("@G", GOLD) for a in argv], _text(fixture))
    assert res.setup_error is None and res.error is None, (res.setup_error, res.error)
    with gzip.open(os.path.join(GOLD, "filter", name + ".out.gz"), "rb") as f:
        want = f.read()
    if "randomAllele" in argv:
        assert res.matches(want)
        assert len(res.rows) == want.count(b"\n") - 1
    else:
        assert res.data() == want


@pytest.mark.parametrize("name,text,argv,line", HANGS, ids=[h[0] for h in HANGS])
def test_oracle_names_the_line_the_reference_raises_on(name, text, argv, line):
    res = filter_reference(argv, text)
    assert res.error is not None and res.error[0] == line, res.error
