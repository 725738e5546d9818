#!/usr/bin/env python3
"""Which min-cut solver takes which expansion move, recorded ONCE on an MI355X at the commit before the routing moved into
csrc/move_route.h: tests/golden/expansion_routes_v1.json, replayed by tests/test_gpu_routes.py.  The cases and what is recorded
of each are in tests/route_cases.py.

Every case runs twice; a field is kept only where both runs agree, and a field that does not agree is named in the file's header
("dropped").  The label hash, the energy, the cycle count and the six expansion_paths entries may not be dropped: if one of them
is not reproducible the script stops without writing.  Run from the repository root (about a minute):
    python tests/golden/make_golden_routes.py [output.json [commit]]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import route_cases  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "expansion_routes_v1.json")


def main():
    out, dropped = {}, []
    for case_id in route_cases.cases():
        a, b = (route_cases.flatten(route_cases.run_case(case_id)) for _ in range(2))
        assert a.keys() == b.keys()
        differ = sorted(k for k in a if a[k] != b[k])
        for k in differ:
            print(f"{case_id}: {k} is not reproducible: {a[k]!r} then {b[k]!r}", flush=True)
        if any(route_cases.must_keep(k) for k in differ):
            sys.exit(f"{case_id}: a field that may not be dropped differs between two runs of the same commit; nothing written")
        dropped += [f"{case_id}:{k}" for k in differ]
        out[case_id] = {k: v for k, v in a.items() if k not in differ}
        print(f"{case_id}: {len(out[case_id])} fields", flush=True)
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"      # (an exported tree: the caller names the commit)
    header = {"recorded_at_commit": commit, "runs_per_case": 2, "dropped": dropped,
              "fields": "tests/route_cases.py: flatten() of run_case(); kept where both runs agree"}
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump({"header": header, "cases": out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} cases, dropped {len(dropped)} fields")


if __name__ == "__main__":
    main()
