#!/usr/bin/env python3
"""What a scoring launch decides and produces, recorded ONCE on an MI355X at the commit before the launch decisions moved into
csrc/score_plan.h: tests/golden/score_plans_v1.json, replayed by tests/test_gpu_score_plans.py.  The cases and what is recorded of
each are in tests/score_plan_cases.py.

Every case runs twice; a field is kept only where both runs agree, and a field that does not agree is named in the file's header
("dropped").  Path, filter level and the result digests may not be dropped: if one of them is not reproducible the script stops
without writing.  A geometry case whose result digests are not its default twin's stops it too.  Run from the repository root:
    python tests/golden/make_golden_score_plans.py [output.json [commit]]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import score_plan_cases  # noqa: E402
from pyprogressivex import _lib  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "score_plans_v1.json")


def main():
    out, dropped = {}, []
    ctx = _lib.Context(0)
    try:
        for case_id in score_plan_cases.cases():
            a, b = (score_plan_cases.run_on(ctx, case_id) for _ in range(2))
            assert a.keys() == b.keys()
            differ = sorted(k for k in a if a[k] != b[k])
            for k in differ:
                print(f"{case_id}: {k} is not reproducible: {a[k]!r} then {b[k]!r}", flush=True)
            if any(score_plan_cases.must_keep(k) for k in differ):
                sys.exit(f"{case_id}: a field that may not be dropped differs between two runs of the same commit; nothing written")
            dropped += [f"{case_id}:{k}" for k in differ]
            out[case_id] = {k: v for k, v in a.items() if k not in differ}
    finally:
        ctx.close()
    for case_id, twin in score_plan_cases.GEOMETRY_TWINS.items():
        for k in score_plan_cases.DIGESTS:
            if out[case_id].get(k) != out[twin].get(k):
                sys.exit(f"{case_id}: {k} is not the default geometry's; nothing written")
    paths = sorted({(c["path"], c["filter"]) for c in out.values()})
    print(f"paths and filter levels recorded: {paths}")
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"      # (an exported tree: the caller names the commit)
    header = {"recorded_at_commit": commit, "runs_per_case": 2, "dropped": dropped,
              "fields": "tests/score_plan_cases.py: run_on(); kept where both runs agree"}
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump({"header": header, "cases": out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} cases, dropped {len(dropped)} fields")


if __name__ == "__main__":
    main()
