"""Runs windowStats.py jobs one after another in ONE process (tests/test_gpu_wstats.py starts it under a time limit): a device context
costs a fraction of a second, a Python start with NumPy more, and the goldens are three dozen command lines per input form.

    python tests/wstats_runner.py JOBS.json RESULTS.json

JOBS: [{"argv": [...], "env": {NAME: value}}]; every job should carry `-o`.  RESULTS: per job {"status": exit status, "info": the
run's counters (wstats.last_info), "stderr": what the driver wrote there}.  A job's environment is set for that job alone."""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from genomics_general_amd import wstats
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    results = []
    for job in jobs:
        saved = {k: os.environ.get(k) for k in job.get("env", {})}
        os.environ.update(job.get("env", {}))
        err = io.StringIO()
        wstats.last_info.clear()
        try:
            with contextlib.redirect_stderr(err):
                status = wstats.main(job["argv"]) or 0
        except SystemExit as exc:
            status = exc.code if isinstance(exc.code, int) else (0 if exc.code is None else 1)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        results.append({"status": status, "info": dict(wstats.last_info), "stderr": err.getvalue()})
    with open(sys.argv[2], "w") as f:
        json.dump(results, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
