"""How should the surviving steps of the group-major kernel be handed to the machine?  CPU emulation (numpy, nothing measured on a
GPU) of the metric batch (1e6 pose correspondences x 2048 hypotheses), behind the work lists of csrc/score_worklist.h:
  * the k-d order of the points (median splits of the widest box-normalised dimension, the 3-D part weighted 0.25), the shipped
    group bound (as scripts/analysis_cull_bound.py emulates it, f64, no inflation) and the locality order of the batch;
  * per (group, hypothesis word): the surviving steps, the dense steps (>= 32 candidates of 64, evaluated in place) and the queued
    pairs - a candidate being a pair within 1.05 T2 of the model (a stand-in for the f32 pre-filter);
  * a wave's cost: 2.1 us + 0.25 us per staged word + 0.255 us per filter step + 0.55 us per dense step + 0.6 us per 64 queued pairs
    (the phase timers of docs/lab-notebook.md, "Trimming the group-major step loop"); a wave that finds nothing: 0.3 us;
  * list scheduling of the waves over SLOTS wave slots in dispatch order.
usage: python scripts/analysis_group_items.py [slots [item widths ...]]      (defaults: 5400 slots, widths 2 4 8)
Output of the committed run (22 s; docs/lab-notebook.md, "A heavy-first work list", has the table next to the measured times):
1 427 604 surviving steps (device: 1.417 M), survivors in 6.8 of a group's 32 words, 43 977 non-empty 4-word items; today's
5 strided parts in group order 126 us with a 21 us tail; 4-word items in 4 classes 16 / 48 / 128 heaviest first 105 us, tail 7;
sorted by weight 102.  Re-run to price another item width, class count or set of thresholds."""
import heapq
import os
import sys
import time

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'progressive-x_amd')]
import numpy as np
from pyprogressivex import datasets

SLOTS = int(sys.argv[1]) if len(sys.argv) > 1 else 5400
WIDTHS = [int(a) for a in sys.argv[2:]] or [2, 4, 8]
THRESHOLDS = {4: ((16, 48, 128), (24, 64, 160), (32, 96, 192)), 2: ((32,), (64,))}      # per class count, for 4-word items
C_WAVE, C_WORD, C_STEP, C_DENSE, C_QUEUE, C_EMPTY = 2.1, 0.25, 0.255, 0.55, 0.6 / 64, 0.3

x1, x2, K, lab, gt = datasets.make_poses(n_per_object=50000, n_objects=16, n_outliers=200000, seed=0)
pts, f = datasets.normalize_pnp(x1, x2, K)
thr = 4.0 / f; T2 = 9.0 / 4.0 * thr * thr; T = np.sqrt(T2)
hyps = datasets.make_pose_hypotheses(gt, M=2048, seed=1)
n, d = pts.shape
M = len(hyps)


def kd_order(X, leaf=64):
    order = np.arange(len(X))
    stack = [(0, len(X))]
    while stack:
        a, b = stack.pop()
        m = b - a
        if m <= leaf:
            continue
        sub = X[order[a:b]]
        k = int(np.argmax(sub.max(0) - sub.min(0)))
        nl = ((m // leaf) // 2) * leaf if (m // leaf) >= 2 else leaf
        if nl == 0 or nl >= m:
            nl = (m // 2 // leaf) * leaf or leaf
        idx = np.argpartition(sub[:, k], nl - 1)
        order[a:b] = order[a:b][idx]
        stack.append((a, a + nl)); stack.append((a + nl, b))
    return order


def spread16(x):
    x = x & 0xffff
    x = (x | (x << 8)) & 0x00ff00ff
    x = (x | (x << 4)) & 0x0f0f0f0f
    x = (x | (x << 2)) & 0x33333333
    return (x | (x << 1)) & 0x55555555


t_start = time.time()
scale = 1.0 / (pts.max(0) - pts.min(0)); scale[2:5] *= 0.25
sp = pts[kd_order(pts * scale)]
G = (n + 63) // 64
pad = G * 64 - n
spp = np.concatenate([sp, np.repeat(sp[-1:], pad, 0)]) if pad else sp          # the tail group repeats its last row
grp = spp.reshape(G, 64, d)
# the locality order of the batch (capi.hip locality_keys): Morton code of the projected object origin
kx, ky = hyps[:, 3] / hyps[:, 11], hyps[:, 7] / hyps[:, 11]
qx = ((kx - kx.min()) / (kx.max() - kx.min()) * 65535.0).astype(np.int64); qy = ((ky - ky.min()) / (ky.max() - ky.min()) * 65535.0).astype(np.int64)
P = hyps[np.argsort(spread16(qx) | (spread16(qy) << 1), kind='stable')].reshape(-1, 3, 4)
W = M // 64
# ---- the group bound, all (group, hypothesis) pairs
X = grp[:, :, 2:5]
c = 0.5 * (X.min(1) + X.max(1)); rho = np.sqrt(((X - c[:, None]) ** 2).sum(2).max(1))
ub = 0.5 * (grp[:, :, 0].min(1) + grp[:, :, 0].max(1)); vb = 0.5 * (grp[:, :, 1].min(1) + grp[:, :, 1].max(1))
ru = np.abs(grp[:, :, 0] - ub[:, None]).max(1); rv = np.abs(grp[:, :, 1] - vb[:, None]).max(1)
nrm = np.linalg.norm(P[:, :, :3], axis=2)
steps = np.zeros((G, W), np.int64); dense = np.zeros((G, W), np.int64); queued = np.zeros((G, W), np.int64)
for g0 in range(0, G, 512):
    s = slice(g0, min(g0 + 512, G))
    cc = np.einsum('mij,gj->gmi', P[:, :, :3], c[s]) + P[None, :, :, 3]                    # [g, m, 3]
    dx, dy, dz = (nrm[None, :, k] * rho[s, None] for k in range(3))
    zs = np.abs(cc[..., 2]) + dz
    ex = np.abs(ub[s, None] * cc[..., 2] - cc[..., 0]); ey = np.abs(vb[s, None] * cc[..., 2] - cc[..., 1])
    mx = ru[s, None] * zs + np.abs(ub[s, None]) * dz + dx; my = rv[s, None] * zs + np.abs(vb[s, None]) * dz + dy
    keep = ~((ex - mx > T * zs) | (ey - my > T * zs))
    gi, mi = np.nonzero(keep)
    for a in range(0, len(gi), 200000):                                                  # the f32 filter's candidates per step
        g_, m_ = gi[a:a + 200000] + g0, mi[a:a + 200000]
        pr = np.einsum('kij,knj->kni', P[m_, :, :3], grp[g_][:, :, 2:5]) + P[m_, None, :, 3]
        r2 = (grp[g_][:, :, 0] - pr[..., 0] / pr[..., 2]) ** 2 + (grp[g_][:, :, 1] - pr[..., 1] / pr[..., 2]) ** 2
        nc = (r2 < 1.05 * T2).sum(1)
        np.add.at(steps, (g_, m_ // 64), 1)
        np.add.at(dense, (g_, m_ // 64), nc >= 32)
        np.add.at(queued, (g_, m_ // 64), np.where(nc < 32, nc, 0))
print(f"emulated in {time.time() - t_start:.0f} s: {steps.sum()} surviving steps, {dense.sum()} dense, {queued.sum()} queued pairs; "
      f"a group has survivors in {np.count_nonzero(steps, axis=1).mean():.1f} of its {W} words")


def cost(sel_words, st, de, qu):
    """us of a wave that stages `sel_words` non-empty words with st steps, de of them dense, and qu queued pairs"""
    return np.where(st > 0, C_WAVE + C_WORD * sel_words + C_STEP * st + C_DENSE * de + C_QUEUE * qu, C_EMPTY)


def makespan(costs, slots=SLOTS):
    """list scheduling in dispatch order: (makespan, tail = makespan - the time the last wave starts, sum of the work)"""
    free = [0.0] * slots
    heapq.heapify(free)
    end = last_start = 0.0
    for cst in costs:
        t0 = heapq.heappop(free)
        last_start = t0
        heapq.heappush(free, t0 + cst)
        end = max(end, t0 + cst)
    return end, end - last_start, float(np.sum(costs))


def items(width):
    cols = (W + width - 1) // width
    padw = cols * width - W
    def fold(a):
        a = np.concatenate([a, np.zeros((G, padw), a.dtype)], 1) if padw else a
        return a.reshape(G, cols, width)
    st, de, qu = fold(steps), fold(dense), fold(queued)
    return (st > 0).sum(2), st.sum(2), de.sum(2), qu.sum(2)


def report(name, costs):
    costs = np.asarray(costs, float)
    live = costs[costs > C_EMPTY]
    end, tail, work = makespan(costs)
    print(f"{name:68s} waves {len(costs):7d} (empty {np.sum(costs <= C_EMPTY):6d})  makespan {end:6.1f} us  tail {tail:5.1f}  work/slots {work / SLOTS:6.1f}  "
          f"life mean {live.mean():4.1f} p90 {np.percentile(live, 90):4.1f} p99 {np.percentile(live, 99):4.1f} max {live.max():4.1f}")


# today: 5 strided parts per group, group order (co-located mapping: XCD g & 7 takes its groups in order - one queue here)
parts = []
for p in range(5):
    sel = slice(p, W, 5)
    parts.append(cost((steps[:, sel] > 0).sum(1), steps[:, sel].sum(1), dense[:, sel].sum(1), queued[:, sel].sum(1)))
report("today: 5 strided parts per group, group order", np.stack(parts, 1).ravel())
even = cost(np.count_nonzero(steps, axis=1) / 5.0, steps.sum(1) / 5.0, dense.sum(1) / 5.0, queued.sum(1) / 5.0)
report("a group's steps split evenly over its 5 waves, group order", np.repeat(even, 5))
for width in WIDTHS:
    nw, st, de, qu = items(width)
    cst = cost(nw, st, de, qu)
    live = st > 0
    if width == 4:
        report("items of 4 words, non-empty only, group order", cst[live])
    scale_t = width / 4.0
    for classes, ts in THRESHOLDS.items():
        for t in ts:
            t = tuple(int(x * scale_t) for x in t)
            cls = sum((st >= x).astype(int) for x in t)
            order = np.argsort(-cls[live], kind='stable')                                  # heaviest class first, list order inside
            report(f"items of {width} words, {classes} classes {t}, heaviest first", cst[live][order])
    report(f"items of {width} words, sorted by weight (the bound of any class count)", cst[live][np.argsort(-st[live], kind='stable')])
