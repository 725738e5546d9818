#!/usr/bin/env python3
"""splitComponents' measurements: pgx_label_components next to the graph build every call pays anyway, on make_planes scenes (six
planes, half of the points uniform outliers, 1 cm noise, points in random order) of 10^4, 10^5 and 10^6 points with the PLANTED
labels, for the k-NN graph at k = 16 and for a ball graph whose radius is bisected to a mean row length of about 30.

Times are device-event times (pgx_timer_start / pgx_timer_stop on the context's stream) around calls that end in a stream
synchronisation, after `--warmup` calls, `--reps` repetitions: median, minimum and maximum.  The components call is upload of the labels
(4 n bytes) + five launches + read-back (4 n bytes, then 12 bytes per component).  The launches alone - the hook launch among them - come
from a second run of this script under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/bench_components.py
--kernel-run`, merged with `--merge DIR` (per-dispatch durations of cc_init_kernel, cc_hook_kernel, cc_flatten_kernel and
cc_fill_kernel: the --kernel-run launches warmup + reps of each per configuration, in the order of the first run).  The host model's
wall time (tests/components_model.py, a breadth-first search in Python) is taken at 10^4 and 10^5 and its result compared with the
device's.  The largest tree depth seen in the hook launch is not recorded: parent[] never leaves the device.  Writes
profiles/components_bench.json and prints it.

usage: bench_components.py [--sizes 10000,100000,1000000] [--warmup 2] [--reps 9] [--out FILE] [--kernel-run | --merge DIR]"""
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
from pyprogressivex import _lib, datasets  # noqa: E402

PLANES = 6
KERNELS = ("cc_init_kernel", "cc_hook_kernel", "cc_flatten_kernel", "cc_fill_kernel")
MODEL_MAX_N = 100000


def scene(n, seed=2):
    p, gen, _ = datasets.make_planes(n_per_plane=n // (2 * PLANES), n_planes=PLANES, n_outliers=n - PLANES * (n // (2 * PLANES)), seed=seed)
    order = np.random.default_rng(0).permutation(len(p))
    labels = np.where(gen > 0, gen - 1, PLANES).astype(np.int32)            # findPlanes' convention: the outliers get the label K
    return np.ascontiguousarray(p[order]), np.ascontiguousarray(labels[order])


def timed(ctx, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), reps=reps)


def ball_radius(ctx, pts, want=30.0):
    """a radius whose ball graph has a mean row length within 10 % of `want`: from the mean spacing of the inliers on 96 square units of
    patches, scaled by sqrt(want / mean row) by at most 1.5 a step, so that no step builds a graph much larger than the one wanted"""
    n = len(pts)
    r = 3.0 * np.sqrt(96.0 / (n / 2))
    for _ in range(24):
        deg = ctx.graph_build(pts, _lib.GRAPH_BALL, radius=r, fetch=False) / n
        if abs(deg - want) <= 0.1 * want:
            break
        r *= float(np.clip(np.sqrt(want / max(deg, 1e-3)), 1.0 / 1.5, 1.5))
    return r


def configurations(ctx, pts):
    r = ball_radius(ctx, pts)
    return [("knn k=16", _lib.GRAPH_KNN, 0.0, 16), (f"ball r={r:.4g}", _lib.GRAPH_BALL, r, 1)]


def merge(path, trace_dir, warmup, reps):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = [r for f in sorted(files) for r in csv.DictReader(open(f))]
    col = {key.lower(): key for key in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    rec = json.load(open(path))
    keys = [(s, c) for s in rec["sizes"] for c in rec["sizes"][s]["graphs"]]
    per = warmup + reps
    for kernel in KERNELS:
        durs = [(int(r[t0]), (int(r[t1]) - int(r[t0])) / 1e3) for r in rows if kernel in r[name]]
        durs = [d for _, d in sorted(durs)]
        if len(durs) != per * len(keys):
            raise SystemExit(f"{len(durs)} dispatches of {kernel} in the trace, {per * len(keys)} expected")
        for j, (s, c) in enumerate(keys):
            d = durs[j * per + warmup:(j + 1) * per]
            rec["sizes"][s]["graphs"][c].setdefault("kernels_us", {})[kernel] = dict(
                median=float(np.median(d)), min=float(min(d)), max=float(max(d)), dispatches=len(d), source="rocprofv3 --kernel-trace")
    text = json.dumps(rec)
    open(path, "w").write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    ap.add_argument("--kernel-run", action="store_true", help="only the pgx_label_components calls, for a kernel trace; writes nothing")
    ap.add_argument("--merge", default=None, help="directory of the kernel trace to merge into --out")
    args = ap.parse_args()
    if args.merge:
        return merge(args.out, args.merge, args.warmup, args.reps)
    ctx = _lib.Context(int(os.environ.get("PGX_DEVICE", "0")))
    out = dict(workload="components", device=ctx.device_info()["name"], warmup=args.warmup,
               timing="device events on the context's stream around calls that end in a stream synchronisation; components call = upload "
                      "4 n B + five launches + read-back 4 n B + 12 B per component",
               tree_depth="not recorded: parent[] never leaves the device", sizes={})
    for size in [int(s) for s in args.sizes.split(",") if s]:
        pts, labels = scene(size)
        n = len(pts)
        graphs = {}
        for tag, kind, radius, k in configurations(ctx, pts):
            arcs = ctx.graph_build(pts, kind, radius=radius, k=k, fetch=False)
            if args.kernel_run:
                for _ in range(args.warmup + args.reps):
                    ctx.label_components(labels, PLANES)
                graphs[tag] = {}
                continue
            g = dict(arcs=int(arcs), mean_row=arcs / n)
            g["graph_build"] = timed(ctx, lambda: ctx.graph_build(pts, kind, radius=radius, k=k, fetch=False), args.warmup, args.reps)
            g["components_call"] = timed(ctx, lambda: ctx.label_components(labels, PLANES), args.warmup, args.reps)
            comp, first, sizes = ctx.label_components(labels, PLANES)
            off = ctx.graph_fetch()[0]
            g.update(components=int(len(first)), largest=int(sizes.max()) if len(sizes) else 0, of_ten_points_or_more=int((sizes >= 10).sum()),
                     longest_row=int(np.diff(off).max()), rows_beyond_the_threshold=int((np.diff(off) > _lib.COMPONENTS_LONG_ROW).sum()))
            if n <= MODEL_MAX_N:
                import components_model as CM
                off, idx, _ = ctx.graph_fetch()
                t0 = time.perf_counter()
                ref = CM.label_components(off, idx, labels, PLANES)
                g["host_model_s"] = time.perf_counter() - t0
                g["equals_host_model"] = bool(all(np.array_equal(a, b) for a, b in zip((comp, first, sizes), ref)))
            graphs[tag] = g
            print(size, tag, g, file=sys.stderr, flush=True)
        out["sizes"][str(size)] = dict(n=n, graphs=graphs)
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
