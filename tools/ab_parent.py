"""A host-side refactoring against the library of its parent commit, on one GPU:
    python tools/ab_parent.py PARENT_LIBRARY OUT_DIR [SECONDS]
(1) rocprofv3 --kernel-trace of six bench workloads on the parent's library (PG_LIBRARY) and on this tree's: kernel names, grid sizes,
workgroup sizes and LDS bytes, in dispatch order, must be equal; (2) fresh bench.py processes, parent against this tree, four rounds in
alternating order, with the parent's own spread as the yardstick; the arrays dumped in the first round are compared byte for byte.
Every process runs under its own time limit, nothing is started after one failed, and no round is begun that would end after SECONDS."""
import csv, glob, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT, OUT = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
T0 = time.time()
DEADLINE = float(sys.argv[3]) if len(sys.argv) > 3 else 1150.0
WORK = [("northstar", {}), ("c2", {}), ("c4", {}), ("c3", {}), ("popfreq", {}), ("c2", {"PG_PAIR_VALU": "1"})]
os.makedirs(OUT, exist_ok=True)
log = open(os.path.join(OUT, "log.txt"), "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


def wname(w, env):
    return w + ("[%s]" % ",".join("%s=%s" % kv for kv in env.items()) if env else "")


def run(cmd, env, limit, tag):
    e = dict(os.environ, **env)
    t = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=e, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    say("  %s: rc %d, %.1f s (at %.0f s)" % (tag, r.returncode, time.time() - t, time.time() - T0))
    if r.returncode != 0:
        say(r.stdout.decode()[-1500:])
        say(r.stderr.decode()[-3000:])
        say("STOP: a process failed; nothing more is started")
        sys.exit(1)
    return r.stdout.decode()


def trace_rows(d):
    files = glob.glob(os.path.join(glob.escape(d), "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        return None, "kernel_trace.csv files: %r" % files
    with open(files[0]) as f:
        rows = list(csv.DictReader(f))
    keys = [k for k in rows[0] if k == "Kernel_Name" or k.startswith("Grid_Size") or k.startswith("Workgroup_Size") or k.startswith("LDS_Block_Size")]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [tuple(r[k] for k in keys) for r in rows], keys


def bench_cmd(w, extra):
    return [sys.executable, "bench.py", "--gpus", "1", "--workload", w, "--no-tiers", "--no-cpu-baseline"] + extra


# ---- 1. kernel traces ----
say("== kernel traces (rocprofv3 --kernel-trace, --steps 3 --warmup 1)")
trace_ok = True
for w, env in WORK:
    got = {}
    for lib in ("parent", "child"):
        d = os.path.join(OUT, "trace", wname(w, env), lib)
        os.makedirs(d, exist_ok=True)
        e = dict(env)
        if lib == "parent":
            e["PG_LIBRARY"] = PARENT
        run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "--output-format", "csv", "--"] + bench_cmd(w, ["--steps", "3", "--warmup", "1"]), e, 240,
            "trace %s %s" % (wname(w, env), lib))
        got[lib] = trace_rows(d)
    (pa, ka), (ch, kc) = got["parent"], got["child"]
    if pa is None or ch is None:
        say("  %s: no trace: %s %s" % (wname(w, env), ka, kc)); trace_ok = False; continue
    same = pa == ch
    say("  %-22s %d / %d dispatches, columns %s: %s" % (wname(w, env), len(pa), len(ch), ",".join(ka), "EQUAL in order" if same else "DIFFERENT"))
    if not same:
        trace_ok = False
        say("    as multisets: %s" % ("equal" if sorted(pa) == sorted(ch) else "different"))
        for i, (a, b) in enumerate(zip(pa, ch)):
            if a != b:
                say("    first difference at dispatch %d:\n      parent %r\n      child  %r" % (i, a, b)); break
    for lib in ("parent", "child"):                                  # keep only the comparison, not the traces
        for f in glob.glob(os.path.join(glob.escape(os.path.join(OUT, "trace", wname(w, env), lib)), "**", "*"), recursive=True):
            if os.path.isfile(f): os.remove(f)
say("kernel traces:", "all equal" if trace_ok else "NOT all equal")

# ---- 2. A/B ----
say("== A/B (bench.py --steps 20 --warmup 5, fresh processes)")
res = {}
rounds_done = 0
round_s = 0.0
for rnd in range(4):
    if time.time() - T0 + round_s > DEADLINE:
        say("deadline: stopping before round", rnd); break
    t_round = time.time()
    for w, env in WORK:
        order = ("parent", "child") if rnd % 2 == 0 else ("child", "parent")
        for lib in order:
            e = dict(env)
            if lib == "parent":
                e["PG_LIBRARY"] = PARENT
            extra = ["--steps", "20", "--warmup", "5"]
            dd = os.path.join("/tmp", "pp_dump", wname(w, env), lib)
            if rnd == 0:
                os.makedirs(dd, exist_ok=True)
                extra += ["--dump-outputs", dd]
            out = run(bench_cmd(w, extra), e, 150, "round %d %s %s" % (rnd, wname(w, env), lib))
            j = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            x = j.get("extra", j)
            ms = j.get("ms_per_step", x.get("ms_per_step"))
            res.setdefault(wname(w, env), {}).setdefault(lib, []).append((ms, x.get("kernel_ms_per_step", {})))
        if rnd == 0:
            import filecmp
            pd_, cd_ = (os.path.join("/tmp", "pp_dump", wname(w, env), l) for l in ("parent", "child"))
            names = sorted(os.listdir(pd_))
            same = names == sorted(os.listdir(cd_)) and all(filecmp.cmp(os.path.join(pd_, n), os.path.join(cd_, n), shallow=False) for n in names)
            say("  dumped arrays %s: %d files, %s" % (wname(w, env), len(names), "byte-identical" if same else "DIFFERENT"))
    rounds_done = rnd + 1
    round_s = time.time() - t_round
    with open(os.path.join(OUT, "ab_raw.json"), "w") as f:
        json.dump(res, f)

say("== summary (%d rounds)" % rounds_done)
for name, r in res.items():
    p = [v[0] for v in r["parent"]]; c = [v[0] for v in r["child"]]
    say("# %-22s ms_per_step parent %s  median %.4f spread %.4f | child %s median %.4f (%+.4f)%s" % (
        name, " ".join("%.4f" % v for v in p), statistics.median(p), max(p) - min(p), " ".join("%.4f" % v for v in c), statistics.median(c),
        statistics.median(c) - statistics.median(p), "" if min(p) <= statistics.median(c) <= max(p) else (" below (faster)" if statistics.median(c) < min(p) else " ABOVE")))
    for k in r["parent"][0][1]:
        pk = [v[1].get(k) for v in r["parent"]]; ck = [v[1].get(k) for v in r["child"]]
        if None in pk or None in ck or max(pk) < 0.01: continue
        m = statistics.median(ck)
        say("#     %-16s parent %s [%.4f .. %.4f] | child %s median %.4f %s" % (
            k, " ".join("%.4f" % v for v in pk), min(pk), max(pk), " ".join("%.4f" % v for v in ck), m,
            "within" if min(pk) <= m <= max(pk) else ("below (faster)" if m < min(pk) else "ABOVE")))
say("total %.0f s" % (time.time() - T0))
