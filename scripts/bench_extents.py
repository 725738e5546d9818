#!/usr/bin/env python3
"""instanceExtents' measurements: pgx_instance_extents on make_primitives scenes (two planes, spheres, cylinders and cones each, half
of the points uniform outliers) of 10^4, 10^5 and 10^6 points with the PLANTED labels - eight instances on type 18 rows - in the
generator's order (runs of one label: whole waves share a row) and in random order (no wave does).

Times are device-event times (pgx_timer_start / pgx_timer_stop on the context's stream) around calls that end in a stream
synchronisation, after `--warmup` calls, `--reps` repetitions: median, minimum and maximum.  The call is upload of the points (24 n
bytes), the labels (4 n) and the frames + one memset + three launches + read-back of 64 bytes per instance.  The copies are not timed
by themselves: they are what the call takes beyond its launches.  The launches alone come from a second run of this script under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
scripts/bench_extents.py --kernel-run`, merged with `--merge DIR` (per-dispatch durations of extents_bounds_kernel,
extents_finalise_kernel and extents_occupancy_kernel: the --kernel-run launches warmup + reps of each per configuration, in the order
of the first run).  The numpy model's wall time (tests/extents_model.py) is taken at 10^4 and 10^5 and its result compared with the
device's bit for bit.  Writes profiles/extents_bench.json and prints it.

usage: bench_extents.py [--sizes 10000,100000,1000000] [--warmup 2] [--reps 9] [--out FILE] [--kernel-run | --merge DIR]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests")]
from pyprogressivex import _extents, _lib, datasets  # noqa: E402

KERNELS = ("extents_bounds_kernel", "extents_finalise_kernel", "extents_occupancy_kernel")
MODEL_MAX_N = 100000
EACH = 2


def scene(n):
    per = n // (2 * 4 * EACH)
    pts, _, _, inst, models = datasets.make_primitives(n_per=per, n_outliers=n - 4 * EACH * per, seed=3, n_each=EACH)
    labels = np.where(inst > 0, inst - 1, len(models)).astype(np.int32)      # the find* convention: the outliers get the label K
    frames, _ = _extents.frames(models, _lib.PRIMITIVE3D)
    return np.ascontiguousarray(pts), labels, frames


def timed(ctx, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), reps=reps)


def configurations(pts, labels):
    order = np.random.default_rng(0).permutation(len(pts))
    return [("generator order", pts, labels), ("random order", np.ascontiguousarray(pts[order]), np.ascontiguousarray(labels[order]))]


def merge(path, trace_dir, warmup, reps):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = [r for f in sorted(files) for r in csv.DictReader(open(f))]
    col = {key.lower(): key for key in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    rec = json.load(open(path))
    keys = [(s, c) for s in rec["sizes"] for c in rec["sizes"][s]["orders"]]
    per = warmup + reps
    for kernel in KERNELS:
        durs = [(int(r[t0]), (int(r[t1]) - int(r[t0])) / 1e3) for r in rows if kernel in r[name]]
        durs = [d for _, d in sorted(durs)]
        if len(durs) != per * len(keys):
            raise SystemExit(f"{len(durs)} dispatches of {kernel} in the trace, {per * len(keys)} expected")
        for j, (s, c) in enumerate(keys):
            d = durs[j * per + warmup:(j + 1) * per]
            rec["sizes"][s]["orders"][c].setdefault("kernels_us", {})[kernel] = dict(
                median=float(np.median(d)), min=float(min(d)), max=float(max(d)), dispatches=len(d), source="rocprofv3 --kernel-trace")
    text = json.dumps(rec)
    open(path, "w").write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extents_bench.json"))
    ap.add_argument("--kernel-run", action="store_true", help="only the pgx_instance_extents calls, for a kernel trace; writes nothing")
    ap.add_argument("--merge", default=None, help="directory of the kernel trace to merge into --out")
    args = ap.parse_args()
    if args.merge:
        return merge(args.out, args.merge, args.warmup, args.reps)
    ctx = _lib.Context(int(os.environ.get("PGX_DEVICE", "0")))
    out = dict(workload="extents", device=ctx.device_info()["name"], warmup=args.warmup,
               timing="device events on the context's stream around calls that end in a stream synchronisation; call = upload 28 n B + "
                      "frames + one memset + three launches + read-back 64 B per instance",
               sizes={})
    for size in [int(s) for s in args.sizes.split(",") if s]:
        pts, labels, frames = scene(size)
        n = len(pts)
        orders = {}
        for tag, p, lab in configurations(pts, labels):
            if args.kernel_run:
                for _ in range(args.warmup + args.reps):
                    ctx.instance_extents(p, lab, frames)
                orders[tag] = {}
                continue
            g = dict(call=timed(ctx, lambda: ctx.instance_extents(p, lab, frames), args.warmup, args.reps))
            got = ctx.instance_extents(p, lab, frames)
            g.update(instances=int(len(frames)), live=int(got["count"].sum()), skipped=int(got["skipped"]),
                     cells=[bin(int(o)).count("1") for o in got["occupancy"]])
            if n <= MODEL_MAX_N:
                import extents_model as EM
                t0 = time.perf_counter()
                ref = EM.extents(p, lab, frames)
                g["host_model_s"] = time.perf_counter() - t0
                g["equals_host_model"] = bool(EM.same(got, ref))
            orders[tag] = g
            print(size, tag, g, file=sys.stderr, flush=True)
        out["sizes"][str(size)] = dict(n=n, orders=orders)
    ctx.close()
    if args.kernel_run:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
