"""The filterGenotypes.py drop-in's device route (k_filt_lines, k_filt_thin) on an MI355X against oracle/filter_oracle.py, not against
the host route, at the shapes where the kernels' wavefront loops and LDS records turn over: selected columns around 64 / 128 / 256
lanes, 1 to 32 populations (bit masks, LDS records; 33 refused), 63 to 200 listed contigs, the LDS limit that decides whether the
device takes the job, thinning over more than 64 and more than 4 096 pods with pods that cross blocks, BGZF input, `.gz` output,
16-allele cells, and the lines the reference raises on in a block other than the first.  Each run is a process of its own under a time
limit; PG_TIMING's counters show which route did the work."""
import gzip
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, ROOT)
from filter_cases import edge_case, edge_files  # noqa: E402

from oracle.filter_oracle import filter_reference  # noqa: E402
from test_filter_cpu import HANGS  # noqa: E402

pytestmark = pytest.mark.gpu

PGF_COUNTS_BYTES = 28                    # sizeof(PgfCounts): one population's record in LDS
LDS_LIMIT = 60 * 1024


def _run(inp, argv, out, device=True, block=None, timeout=300):
    """(exit code, output bytes, stderr, PG_TIMING counters) of one run in a process of its own"""
    env = dict(os.environ, PG_TIMING="1", PG_FILTER_DEVICE="1" if device else "0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "filterGenotypes.py"), "-i", inp, "-o", out] + argv,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=timeout, cwd=ROOT)
    err = r.stderr.decode()
    info = {}
    m = re.search(r"PG_TIMING filter (.*)", err)
    if m:
        for kv in m.group(1).split():
            k, v = kv.split("=", 1)
            info[k] = v
    print("\n%s %s rc=%d %s" % ("device" if device else "host", os.path.basename(inp), r.returncode,
                                  " ".join("%s=%s" % kv for kv in sorted(info.items())
                                           if kv[0].endswith(("blocks", "device", "host", "rows")))))
    got = b""
    if os.path.exists(out):
        with (gzip.open(out, "rb") if out.endswith(".gz") else open(out, "rb")) as f:
            got = f.read()
    return r.returncode, got, err, info


def _case(tmp_path, text, argv, files=None, name="in.geno", bgzf=False):
    d = str(tmp_path)
    argv = edge_files(argv, files or {}, d)
    inp = os.path.join(d, name + (".gz" if bgzf else ""))
    with open(inp, "wb") as f:
        if bgzf:
            from genomics_general_amd import genoio
            f.write(genoio.bgzf_compress(text.encode(), block=7000))
        else:
            f.write(text.encode())
    res = filter_reference(argv, text)                          # (the extra files are read where edge_files wrote them)
    return inp, argv, res


def _equal(res, rc, got, err):
    assert res.setup_error is None and res.error is None, (res.setup_error, res.error)
    assert rc == 0, err[-3000:]
    assert res.matches(got), "differs from the oracle"


def _on_device(info, blocks=1):
    assert int(info.get("blocks_on_device", 0)) >= blocks and int(info.get("device_host_blocks", -1)) == 0, info


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 127, 128, 129, 257, 1000])
def test_selected_samples_across_wavefronts(k, tmp_path):
    text, argv, files = _case_args(3000 + k, n_samples=k + 9, n_select=k, n_lines=120 if k < 500 else 60)
    inp, argv, res = _case(tmp_path, text, argv, files)
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), block=2000 + 40 * k)
    _equal(res, rc, got, err)
    _on_device(info)                  # (one block when the option set thins in a pod longer than the file: pods stay whole)


def _case_args(seed, **shape):
    """edge_case at the shape: the first seed from `seed` on whose option set writes rows"""
    for s in range(seed, seed + 50):
        text, argv, files = edge_case(s, **shape)
        if filter_reference(argv, text, files={"@D/" + k: v for k, v in files.items()}).rows:
            break
    return text, argv, files


@pytest.mark.parametrize("k", [1, 2, 31, 32])
def test_populations_up_to_the_bit_mask_width(k, tmp_path):
    text, argv, files = _case_args(3100 + k, n_samples=40, n_lines=150, n_pops=k, shared=True, empty_pop=k > 1, ploidy="none")
    assert argv.count("-p") == k
    inp, argv, res = _case(tmp_path, text, argv, files)
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), block=4000)
    _equal(res, rc, got, err)
    _on_device(info)


def test_33_populations_are_refused(tmp_path):
    text, argv, files = edge_case(3133, n_samples=40, n_lines=20, n_pops=33, shared=True, ploidy="none")
    inp, argv, res = _case(tmp_path, text, argv, files)
    rc, _, err, _ = _run(inp, argv, str(tmp_path / "o.geno"))
    assert rc != 0 and "more than 32 populations" in err, err[-2000:]


@pytest.mark.parametrize("listing", ["--include", "--exclude"])
@pytest.mark.parametrize("k", [63, 64, 65, 200])
def test_listed_contigs_across_a_wavefront(k, listing, tmp_path):
    text, argv, files = _case_args(3200 + k, n_samples=6, n_lines=400, n_contigs=90, n_listed=k, listing=listing, ploidy="none")
    assert argv.index(listing) >= 0
    inp, argv, res = _case(tmp_path, text, argv, files)
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), block=5000)
    _equal(res, rc, got, err)
    _on_device(info, 2)


@pytest.mark.parametrize("over", [0, 1])
def test_header_width_at_the_lds_limit(over, tmp_path):
    """n_cols * 4 + n_pops * sizeof(PgfCounts) <= 60 KiB: the device takes the job; one column more: the host does it all"""
    n_pops = 2
    n_cols = (LDS_LIMIT - n_pops * PGF_COUNTS_BYTES) // 4 + over
    n = n_cols - 2
    names = ["w%d" % j for j in range(n)]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    for i in range(12):
        rows.append("\t".join(["sc1", str(i + 1)] + [("ACGT"[(i + j) % 4] + "/" + "AC"[(i * j) % 2]) if (i + j) % 13 else "N/N"
                                                      for j in range(n)]))
    text = "\n".join(rows) + "\n"
    argv = ["-p", "P0", ",".join(names[0::3]), "-p", "P1", ",".join(names[1::3]), "--keepAllSamples", "--minPopCalls", "1",
            "-s", ",".join(names[::-1][:300] + names[:-300])]
    inp, argv, res = _case(tmp_path, text, argv)
    assert n_cols * 4 + n_pops * PGF_COUNTS_BYTES == LDS_LIMIT + 4 * over
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"))
    _equal(res, rc, got, err)
    if over:
        assert int(info.get("blocks_on_device", 0)) == 0, info
    else:
        _on_device(info)


@pytest.mark.parametrize("pod,block", [(1, 3000), (63, 20000), (64, 3000), (65, 20000), (100000, 3000)])
def test_thinning_over_many_pods_and_blocks(pod, block, tmp_path):
    lines = {1: 5000, 100000: 1500}.get(pod, 4600)
    text, argv, files = _case_args(3300 + pod, n_samples=5, n_lines=lines, n_contigs=6, thin=2, pod=pod, ploidy="none", big_pos=False)
    data = text.split("\n")[1:-1]
    if pod < lines:
        assert lines // pod > 64 or pod == 1
        assert any(data[b].split("\t", 1)[0] != data[b - 1].split("\t", 1)[0] for b in range(pod, lines, pod)), \
            "no scaffold change on a pod boundary"
    inp, argv, res = _case(tmp_path, text, argv, files)
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), block=block)
    _equal(res, rc, got, err)
    _on_device(info, 2 if pod < lines else 1)         # (a pod longer than the file is one block)


@pytest.mark.parametrize("bgzf", [False, True])
@pytest.mark.parametrize("gz_out", [False, True])
def test_plain_and_bgzf_input_plain_and_gz_output(bgzf, gz_out, tmp_path):
    text, argv, files = _case_args(3400, n_samples=70, n_lines=900, ploidy="file", fmt="coded")
    argv = [a for a in argv]
    if "--thinDist" in argv:
        i = argv.index("--thinDist")
        del argv[i:i + 4]
    inp, argv, res = _case(tmp_path, text, argv, files, bgzf=bgzf)
    rc, got, err, info = _run(inp, argv, str(tmp_path / ("o.geno.gz" if gz_out else "o.geno")), block=40000)
    _equal(res, rc, got, err)
    _on_device(info, 2)
    if bgzf:
        assert int(info["blocks_inflated_on_device"]) >= 1, info


def _hap16(seed, n_lines, over_limit=None):
    """16-allele cells (31 bytes phased) in every column"""
    import random
    R = random.Random(seed)
    names = ["p%d" % j for j in range(70)]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    for i in range(n_lines):
        site = R.sample("ACGT", R.randint(1, 4))
        rows.append("\t".join(["sc1", str(i + 1)] + ["/".join(R.choice(site) for _ in range(16)) for _ in names]))
    if over_limit:
        t = rows[over_limit - 1].split("\t")
        t[5] = "|".join("A" * 17)
        rows[over_limit - 1] = "\t".join(t)
    return "\n".join(rows) + "\n"


def test_cells_of_16_alleles_stay_on_the_device(tmp_path):
    inp, argv, res = _case(tmp_path, _hap16(1, 400), ["-of", "coded", "--minAlleles", "2"])
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), block=60000)
    _equal(res, rc, got, err)
    _on_device(info, 2)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_a_cell_of_17_alleles_on_a_later_block_stops_the_run(device, tmp_path):
    text = _hap16(2, 400, over_limit=351)
    inp, argv, res = _case(tmp_path, text, ["-of", "coded"])
    assert res.error is None                      # (the reference takes it: 17 alleles are the drop-in's documented limit)
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), device=device, block=60000)
    assert rc != 0 and "line 351:" in err, err[-2000:]


FILL = {"diplo_in": "N\tN"}


@pytest.mark.parametrize("name,text,argv,line", HANGS, ids=[h[0] for h in HANGS])
def test_lines_the_reference_raises_on_in_a_later_block(name, text, argv, line, tmp_path):
    """300 lines that fail --minCalls before the case's own lines: the line falls in a later block of the device route"""
    head, body = text.split("\n", 1)
    fill = "".join("f\t%d\t%s\n" % (i + 1, FILL.get(name, "N/N\tN/N")) for i in range(300))
    text = head + "\n" + fill + body
    inp, argv, res = _case(tmp_path, text, argv)
    assert res.error is not None and res.error[0] == line + 300, res.error
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), block=1500)
    assert rc != 0 and ("line %d:" % res.error[0]) in err, err[-2000:]


def test_a_line_thinning_drops_does_not_raise(tmp_path):
    """--HWE with populations raises only at a line siteTest sees: thinning drops it first here, and the run succeeds"""
    fill = "".join("f\t%d\tA/A\tA/A\n" % (10 * i + 1) for i in range(300))
    text = "#CHROM\tPOS\ta\tb\n" + fill + "c\t1\tA/A\tA/A\nc\t2\tA/T\tT/T\nc\t50\tA/A\tA/A\n"
    argv = ["--HWE", "0.05", "both", "-p", "P", "a,b", "--thinDist", "10", "--podSize", "7"]
    inp, argv, res = _case(tmp_path, text, argv)
    assert res.error is None and res.rows[-1][:2] == ["c", "50"]
    rc, got, err, info = _run(inp, argv, str(tmp_path / "o.geno"), block=1500)
    _equal(res, rc, got, err)
    _on_device(info, 2)
