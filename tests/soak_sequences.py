"""Random call sequences on ONE context against the model of the C ABI (tests/ctx_model.py): generator, runner, judge.

Every other soak opens a context and makes the same kind of call over and over; the state hand-overs under test elsewhere are the
ones somebody scripted.  Here a sequence is an unscripted history: every single-GPU call of _lib.Context that touches or reads
resident state, in random order, on sizes at which the buffers and paths differ, with the histories that have gone wrong before
drawn more often and, now and then, a call the contract refuses.

  generate(seed)           -> ops, plain data (name, arguments): driven by the true model only, never by a device
  run(ctx, ops)            -> outcomes of the calls on a device context (+ the history-independence checkpoints)
  judge(model, ops, outs)  -> the disagreements between the outcomes and a model that replays the ops

usage: python tests/soak_sequences.py <seed> <sequences>       (sequence k of a run is generate(seed * 1000 + k))"""
import ctypes as C
import os
import re
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "progressive-x_amd"), os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]
import numpy as np
import ctx_model as CM
from ctx_model import ContextModel
from helpers import ALL_MODEL_CASES, make_case
from soak_expansion import odd_graph, odd_unary
from soak_pointwise import wild_models
import pgx_oracle as O

REL = 1e-9                                      # tests/test_gpu_switches.py: floating sums against the oracle
N_LIST = [1, 63, 64, 65, 257, 1025, 2500]       # labelling stays at n <= 2500: the oracle's Dinic solver is the slow side
M_LIST = [1, 64, 65, 257]
MAX_LABELS = 7
OPS_PER_SEQUENCE = 80
P_REFUSED = 0.2
MAX_CHECKPOINTS = 8
NORM = np.array([0.01, 300.0, 200.0, 0.012, 310.0, 190.0])       # Hartley normalisation of the DLT rows, as tests/test_gpu_switches.py
GRAM_AFFINE, GRAM_DLT_H, GRAM_EPI_F, GRAM_VP, GRAM_PNP_GN, GRAM_SPHERE, GRAM_CIRCLE = range(7)
OP_NAMES = sorted(k[3:] for k in vars(ContextModel) if k.startswith("op_"))
WRITERS = ("set_labels", "expand_alpha", "expansion", "greedy_labeling")
# the computing calls a checkpoint repeats on a fresh context (compound_update / get_preference need the slots' history: not these)
CHECKPOINTED = ("score", "score_fetch", "score_inliers", "score_accumulators", "preference", "pearl_unary", "residual_sum", "residual_sums",
                "bucket", "gc_labeling", "gc_inliers", "epipolar_support", "gram", "gram_labels", "gram_batch", "pnp_refine_batch",
                "solve_minimal", "solve_minimal_sampled", "energy", "expand_alpha", "expansion", "greedy_labeling", "graph_build", "get_compound")

_CASES = {}


def case(name, n, seed):
    key = (name, n, seed)
    if key not in _CASES:
        mt, pts, models, thr = make_case(name, n, 257, seed=seed)
        models = wild_models(np.random.default_rng(seed + 1), models.copy(), 257)
        models[:3] = make_case(name, n, 3, seed=seed)[2]              # the ground truth stays in front
        _CASES[key] = (mt, pts, models, thr)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed, types=None):
        self.rng = np.random.default_rng(seed)
        self.types = list(ALL_MODEL_CASES) if types is None else list(types)
        self.m = ContextModel()
        self.ops, self.outs = [], []
        self.refused = 0
        self.drawn = set()
        self.idx, self.dir = int(self.rng.integers(2, len(N_LIST))), 0          # the sizes walk down, then up, then stay with other points
        self.name = None

    # -- plumbing
    def emit(self, name, **kw):
        out = self.m.step((name, kw))
        assert not (out[0] == "refused" and out[1] is CM.Undrawn), (name, "drew a refusal pgx.h does not document")
        self.ops.append((name, kw))
        self.outs.append(out)
        self.refused += out[0] == "refused"
        return out

    def may_refuse(self, k=1):
        return (self.refused + k) * 5 <= len(self.ops) + k

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    @property
    def T2(self):
        return 2.25 * self.thr * self.thr

    # -- points
    def new_points(self, same_n=False, name=None):
        if not same_n:
            if not 0 <= self.idx + self.dir < len(N_LIST):
                self.dir = -self.dir
            self.idx += self.dir
            self.dir = self.dir or -1
        m = self.m
        had_table, had_weights, had_labels, had_slots, had_rows = (m.prosac is not None, m.weights is not None, m.oc.labels is not None,
                                                                   sorted(m.oc.slots), m.mask_rows is not None)
        self.name = name or (self.name if same_n and self.rng.random() < 0.5 else self.pick(self.types))
        n = N_LIST[self.idx]
        self.mt, self.pts, self.models, self.thr = case(self.name, n, int(self.rng.integers(0, 4)))
        self.emit("set_points", model_type=self.mt, points=self.pts)
        if self.rng.random() < 0.4 and self.may_refuse():               # what the earlier point set left behind is refused, not answered
            menu = [lambda: self.emit("score_fetch", exponent=2, want_masks=False), lambda: self.emit("score_inliers", row=0)]
            if had_rows:
                menu += [lambda: self.emit("score_inliers", row=0)] * 2
            if had_labels:
                menu += [lambda: self.emit("get_labels"), lambda: self.emit("gram", kind=GRAM_AFFINE, sel=("label", 0), params=None, use_weights=False, wpow=2)]
            if had_slots:
                menu += [lambda: self.emit("get_preference", slot=int(had_slots[0]))] * 2
            if had_table and self.mt != CM.NO_SOLVER_TYPE and m.n >= O.SAMPLE_SIZE[self.mt]:
                menu += [lambda: self.emit("solve_minimal_sampled", sampler="prosac", key=5, batch=1, S=1)] * 2
            if had_weights:
                menu += [lambda: self.emit("gram", kind=GRAM_AFFINE, sel=("index", self.index(1)), params=None, use_weights=True, wpow=2)] * 2
            if m.graph_n != m.n:
                menu += [lambda: self.emit("gc_labeling", model=self.models[0].copy(), T2=self.T2, lam=0.2)] * 2
            self.pick(menu)()

    def refused_points(self):
        if self.rng.random() < 0.5:
            self.emit("set_points", model_type=int(self.pick([7, 9])), points=self.pts)
        else:
            self.emit("set_points", model_type=self.mt, points=self.pts[:0])
        self.observe()

    def observe(self):
        """reads that show what a call left behind"""
        k = int(self.rng.integers(0, 7))
        m = self.m
        if k == 0 and m.oc.labels is not None:
            self.emit("get_labels")
        elif k == 1:
            self.emit("get_compound")
        elif k == 2:
            self.emit("graph_size")
        elif k == 3 and m.batch is not None and m.launch is not None and m.launch["batch_id"] == m.batch_id:
            self.emit("score_fetch", exponent=2, want_masks=False)
        elif k == 4 and m.oc.Dq is not None and m.oc.labels is not None:
            self.energy()
        elif k == 5 and m.oc.slots:
            self.emit("get_preference", slot=self.pick(sorted(m.oc.slots)))
        else:
            self.emit("get_labels") if m.oc.labels is not None else self.emit("graph_size")

    # -- scoring
    def batch_models(self):
        M = int(self.pick(M_LIST))
        return np.ascontiguousarray(self.models[self.rng.permutation(257)[:M]])

    def compound(self):
        n = self.m.n
        self.emit("set_compound", compound=None if self.rng.random() < 0.2 else self.rng.random(n) * (self.rng.random(n) < 0.5))

    def score(self):
        self.emit("score", models=self.batch_models(), T2=self.T2, has_compound=bool(self.rng.random() < 0.5), exponent=int(self.pick([1, 2])),
                  want_masks=bool(self.rng.random() < 0.5))

    def upload(self):
        self.emit("score_upload", models=self.batch_models())

    def launch(self, masks=None):
        if self.m.batch is None:
            self.upload()
        self.emit("score_launch", T2=self.T2 * float(self.pick([1.0, 1.0, 4.0])), has_compound=bool(self.rng.random() < 0.5),
                  want_masks=bool(self.rng.random() < 0.5) if masks is None else masks)

    def current(self):
        m = self.m
        return m.batch is not None and m.launch is not None and m.launch["batch_id"] == m.batch_id

    def fetch(self):
        if not self.current():
            self.launch()
        self.emit("score_fetch", exponent=int(self.pick([1, 2])), want_masks=bool(self.m.launch["masks"] and self.rng.random() < 0.6))

    def inliers(self):
        m = self.m
        if not (self.current() and m.mask_rows is not None):
            self.launch(masks=True)
        self.emit("score_inliers", row=int(self.rng.integers(0, m.batch.shape[0])))

    def accumulators(self):
        if self.mt not in CM.ACCUMULATOR_TYPES:
            return self.fetch()
        if self.rng.random() < 0.5:
            self.emit("score_set_global_n", n_total=int(self.pick([0, 50_000_000, 3])))
        self.launch()
        self.emit("score_accumulators")

    def samples(self, S):
        m = O.SAMPLE_SIZE[self.mt]
        s = self.rng.integers(0, self.m.n, (S, m)).astype(np.int32)
        s[:2, 1] = s[:2, 0]                                           # degenerate: NaN rows
        return s

    def solve(self):
        if self.mt == CM.NO_SOLVER_TYPE:
            return self.upload()
        self.emit("solve_minimal", samples=self.samples(int(self.pick([1, 64, 65]))))

    def prosac_table(self):
        n, m = self.m.n, O.SAMPLE_SIZE.get(self.mt, 2)
        count = int(self.pick([64, 65, 130]))
        tops = np.sort(self.rng.integers(min(m, n), n + 1, count)).astype(np.int32) if self.rng.random() < 0.7 else np.full(count, n, np.int32)
        if self.rng.random() < 0.3:
            tops[-3:] = 0                                             # past the convergence bound: uniform over all points
        self.emit("sampler_prosac_set", subset_sizes=tops)

    def sampled(self, sampler=None):
        m = self.m
        if self.mt == CM.NO_SOLVER_TYPE or m.n < O.SAMPLE_SIZE[self.mt]:
            return self.upload()
        sampler = sampler or self.pick(CM.SAMPLERS)
        if sampler == "prosac" and m.prosac is None:
            self.prosac_table()
        if sampler == "napsac" and (m.graph_n != m.n or len(m.oc.graph[1]) == 0):
            self.graph_of_points()
            if len(m.oc.graph[1]) == 0:
                sampler = "uniform"
        S = int(self.pick([1, 64, 65]))
        if sampler == "prosac":
            S = min(S, len(m.prosac))
        self.emit("solve_minimal_sampled", sampler=sampler, key=int(self.rng.integers(1, 1 << 62)), batch=int(self.rng.integers(0, 99)), S=S)

    def radius_range(self):
        lo = float(10.0 ** self.rng.uniform(-2, 1)) * (50.0 if self.name == "circle" else 1.0)
        self.emit("set_radius_range", rmin=lo if self.rng.random() < 0.7 else 0.0, rmax=float(lo * 10.0 ** self.rng.uniform(0, 2)) if self.rng.random() < 0.7 else float("inf"))
        if self.name in ("sphere", "circle"):
            self.solve()

    # -- pointwise
    def preference(self):
        self.emit("preference", model=self.models[int(self.rng.integers(0, 12))].copy(), T2=self.T2, slot=int(self.pick([0, 1, 2, 5])))

    def get_preference(self):
        if not self.m.oc.slots:
            self.preference()
        self.emit("get_preference", slot=self.pick(sorted(self.m.oc.slots)))

    def compound_update(self):
        if not self.m.oc.slots:
            self.preference()
        have = sorted(self.m.oc.slots)
        self.emit("compound_update", slots=[int(s) for s in have[:int(self.rng.integers(0, len(have) + 1))]])

    def pearl(self, K=None, lam=None):
        K = int(self.rng.integers(0, MAX_LABELS)) if K is None else K
        self.emit("pearl_unary", models=np.ascontiguousarray(self.models[:K]), threshold=float(self.thr),
                  lam=float(self.pick([0.0, 0.1, 0.3])) if lam is None else lam)

    def inject(self):
        n, L = self.m.n, int(self.rng.integers(1, MAX_LABELS + 1))
        while True:
            Dq = odd_unary(self.rng, n, L, 0.3)
            if int(Dq.max()) < 1 << 34:                               # (beyond 2^35 the greedy labelling answers PGX_ERR_RANGE)
                break
        self.emit("set_unary_q", Dq=Dq)

    def table(self):
        if self.m.oc.Dq is None:
            self.pearl() if self.rng.random() < 0.7 else self.inject()

    def labels(self, kind=None):
        self.table()
        n, L = self.m.dq_n, self.m.L
        kind = int(self.rng.integers(0, 3)) if kind is None else kind
        lab = np.zeros(n, np.int32) if kind == 0 else self.rng.integers(0, L, n).astype(np.int32) if kind == 1 else np.full(n, L - 1, np.int32)
        self.emit("set_labels", labels=lab)

    def ready(self, lam):
        """a table, labels of its length and range and, for lambda > 0, a graph over its sites"""
        m = self.m
        self.table()
        if m.oc.labels is None or len(m.oc.labels) != m.dq_n or m.labels_max >= m.L:
            self.labels()
        if lam > 0 and m.graph_n != m.dq_n:
            if self.may_refuse() and self.rng.random() < 0.5:             # the graph of an earlier point set is refused, not used
                self.emit("energy", lam=lam, label_cost=1.0)
            self.graph_of_points()

    def lam(self):
        return float(self.pick([0.0, 0.1, 0.3, 0.9]))

    def h(self):
        return float(self.pick([0.0, 0.5, 3.0, 20.0]))

    def energy(self):
        m = self.m
        lam = self.lam() if m.graph_n == m.dq_n else 0.0
        if m.oc.labels is None or len(m.oc.labels) != m.dq_n or m.labels_max >= m.L:
            self.ready(lam)
        self.emit("energy", lam=lam, label_cost=self.h())

    def expand_alpha(self):
        lam = self.lam()
        self.ready(lam)
        self.emit("expand_alpha", lam=lam, label_cost=self.h(), alpha=int(self.rng.integers(0, self.m.L)))
        if self.rng.random() < 0.5:
            self.emit("get_labels")

    def expansion(self, lam=None, h=None, cycles=None):
        lam = self.lam() if lam is None else lam
        self.ready(lam)
        self.emit("expansion", lam=lam, label_cost=self.h() if h is None else h, max_cycles=int(self.pick([1, 2, 1000])) if cycles is None else cycles)

    def greedy(self):
        self.table()
        self.emit("greedy_labeling", label_cost=self.h())

    def label_form(self):
        m = self.m
        if m.oc.labels is None or len(m.oc.labels) != m.n:
            self.emit("set_labels", labels=self.rng.integers(0, 4, m.n).astype(np.int32))
        k = int(self.rng.integers(0, 5))
        top = int(m.oc.labels.max())
        if k == 0:
            self.emit("residual_sum", model=self.models[0].copy(), label=int(self.rng.integers(0, top + 1)))
        elif k == 1:
            self.emit("residual_sums", models=np.ascontiguousarray(self.models[:top + 1]))
        elif k == 2:
            self.emit("bucket", L=top + 1 + int(self.rng.integers(0, 3)))
        elif k == 3:
            kind, prm = self.gram_kind()
            self.emit("gram", kind=kind, sel=("label", int(self.rng.integers(0, top + 1))), params=prm, use_weights=self.use_weights(), wpow=int(self.pick([1, 2])))
        else:
            kind, prm = self.gram_kind()
            K = top + 1
            self.emit("gram_labels", kind=kind, K=K, params=None if prm is None else np.tile(prm, (K, 1)) * (1.0 + 1e-3 * np.arange(K))[:, None],
                      use_weights=self.use_weights(), wpow=int(self.pick([1, 2])))

    # -- fits
    def gram_kind(self):
        d = self.pts.shape[1]
        c, s = self.pts.mean(axis=0), max(float(self.pts.std()), 1.0)
        opts = [(GRAM_AFFINE, None)]
        if d == 2:
            opts.append((GRAM_CIRCLE, np.array([c[0], c[1], s])))
        elif d == 3:
            opts.append((GRAM_SPHERE, np.array([c[0], c[1], c[2], s])))
        elif d == 4:
            opts += [(GRAM_DLT_H, NORM.copy()), (GRAM_EPI_F, NORM.copy()), (GRAM_VP, None)]
        else:
            opts.append((GRAM_PNP_GN, self.models[0].copy()))
        return self.pick(opts)

    def use_weights(self):
        if self.rng.random() < 0.5:
            return False
        if self.m.weights is None:
            self.emit("set_weights", weights=self.rng.random(self.m.n) + 0.5)
        return True

    def weights(self):
        self.emit("set_weights", weights=None if self.rng.random() < 0.25 else self.rng.random(self.m.n) + 0.5)

    def index(self, m):
        n = self.m.n
        return (self.rng.permutation(n)[:m] if m <= n else self.rng.integers(0, n, m)).astype(np.int32)

    def gram_index(self):
        kind, prm = self.gram_kind()
        self.emit("gram", kind=kind, sel=("index", self.index(int(self.pick([1, 14, 65, 300])))), params=prm, use_weights=self.use_weights(),
                  wpow=int(self.pick([1, 2])))

    def gram_batch(self):
        kind, prm = self.gram_kind()
        B, m = int(self.pick([1, 3, 65])), 14
        self.emit("gram_batch", kind=kind, index=np.array([self.index(m) for _ in range(B)]), params=None if prm is None else np.tile(prm, (B, 1)),
                  weights=None if self.rng.random() < 0.5 else self.rng.random(self.m.n) + 0.5, wpow=int(self.pick([1, 2])))

    def pnp_refine(self):
        if N_LIST[self.idx] < 257 or "pnp" not in self.types:
            return self.gram_batch()
        if self.name != "pnp":
            self.new_points(same_n=True, name="pnp")
        with np.errstate(invalid="ignore"):
            inl = np.flatnonzero(O.squared_residuals(self.mt, self.pts, self.models[0]) < self.T2)
        B, m = int(self.pick([1, 3])), 21
        if len(inl) < 2 * m:
            return self.gram_batch()
        picks = np.array([np.sort(self.rng.choice(inl, m, replace=False)) for _ in range(B)]).astype(np.int32)
        inits = np.tile(self.models[0], (B, 1)).reshape(B, 3, 4)
        inits[:, :, 3] += self.rng.normal(0, 0.01, (B, 3))
        self.emit("pnp_refine_batch", inits=inits.reshape(B, 12), index=picks, iterations=10)

    def eigh(self):
        q, B = int(self.pick([3, 9])), int(self.pick([1, 65]))
        X = self.rng.standard_normal((B, 12, q))
        A = np.einsum("bni,bnj->bij", X, X)
        A[::9] *= 1e-12
        self.emit("eigh_smallest_batch", A=A)

    def epipolar(self):
        if "fundamental" not in self.types:
            return self.preference()
        if self.name != "fundamental":
            self.new_points(same_n=True, name="fundamental")
        self.emit("epipolar_support", F=self.models[int(self.rng.integers(0, 3))].copy(), T2=self.T2, S2=self.T2 * 4.0)

    def cut(self):
        m = self.m
        if m.graph_n != m.n:
            self.graph_of_points()
        model, lam = self.models[int(self.rng.integers(0, 6))].copy(), float(self.pick([0.05, 0.14, 0.5, 0.9]))
        self.emit("gc_labeling", model=model, T2=self.T2, lam=lam)
        if self.rng.random() < 0.5:
            self.emit("gc_inliers", model=model, T2=self.T2, lam=lam)

    # -- graphs
    def graph_of_points(self, built=None):
        n = self.m.n
        built = self.rng.random() < 0.6 if built is None else built
        if n < 2 or not built:
            g = odd_graph(self.rng, n)
            return self.emit("set_graph", off=g[0], idx=g[1], mult=g[2])
        kind = int(self.pick([0, 1, 2]))
        k = int(self.pick([1, 3, 5, 6]))
        span = float(np.abs(self.pts).max()) or 1.0
        radius = span * (float(10.0 ** self.rng.uniform(-2, 0)) if kind == 0 else 0.5 / np.sqrt(n))
        while kind == 1 and len(CM.cached(O.graph_build, self.pts, kind, radius=radius, k=k)[1]) > 40000:
            radius *= 0.5
        self.emit("graph_build", points=self.pts, kind=kind, radius=float(radius), k=k)

    def graph_read(self):
        self.emit("graph_fetch") if self.m.oc.graph is not None and self.rng.random() < 0.6 else self.emit("graph_size")

    # -- the histories that have gone wrong before
    def h_identical_expansion(self):
        """the identical expansion call repeated, with and without a writer in between"""
        lam, h = float(self.pick([0.1, 0.3])), self.h()
        self.pearl(K=int(self.rng.integers(1, MAX_LABELS)), lam=lam)
        self.graph_of_points()
        self.labels(kind=0)
        self.expansion(lam, h, 1000)
        k = int(self.rng.integers(0, 4))
        if k == 1:
            self.emit("set_labels", labels=self.m.oc.labels.copy())
        elif k == 2:
            self.emit("expand_alpha", lam=lam, label_cost=h, alpha=int(self.rng.integers(0, self.m.L)))
        elif k == 3:
            self.graph_of_points()                                   # a new graph of the same n between two identical calls
        self.expansion(lam, h, 1000)
        self.emit("get_labels")

    def h_from_zeros_again(self):
        """a from-zeros expansion after one with the same leading models, then a smaller table after moves wrote large labels"""
        lam, h = float(self.pick([0.1, 0.3])), self.h()
        K = int(self.rng.integers(2, MAX_LABELS))
        self.pearl(K=K, lam=lam)
        if self.m.graph_n != self.m.n:
            self.graph_of_points()
        self.labels(kind=0)
        self.expansion(lam, h, int(self.pick([1, 1000])))
        self.labels(kind=0)
        K2 = int(self.pick([K, K, max(1, K - 1), min(MAX_LABELS - 1, K + 1)]))
        if K2 != K or self.rng.random() < 0.5:
            self.pearl(K=K2, lam=lam)
        self.expansion(lam, h, int(self.pick([1, 1, 2])))
        self.emit("get_labels")
        top = int(self.m.oc.labels.max())
        if self.may_refuse(2):
            self.pearl(K=int(self.rng.integers(0, max(1, top))) if self.rng.random() < 0.7 else max(0, K2 - 1), lam=lam)
            self.emit("energy", lam=0.0, label_cost=h)
            self.emit("expansion", lam=0.0, label_cost=h, max_cycles=1)
            self.labels(kind=0)
            self.emit("energy", lam=lam, label_cost=h)

    def h_moves_wrote_nothing(self):
        """moves that MAY have written large labels and wrote none, then a smaller table: the bound is the moves', not the labelling's"""
        n, L = self.m.n, int(self.rng.integers(3, MAX_LABELS + 1))
        Dq = np.full((n, L), 1 << 32, np.int64)
        Dq[:, 0] = 0                                                  # label 0 is free, every other label costs 1: no move relabels a site
        self.emit("set_unary_q", Dq=Dq)
        self.emit("set_labels", labels=np.zeros(n, np.int32))
        if self.rng.random() < 0.5:
            self.emit("expansion", lam=0.0, label_cost=self.h(), max_cycles=int(self.pick([1, 2, 1000])))
        else:
            self.emit("expand_alpha", lam=0.0, label_cost=self.h(), alpha=L - 1)
        self.emit("set_unary_q", Dq=np.ascontiguousarray(Dq[:, :L - 1]))
        if self.may_refuse(2):
            self.emit("energy", lam=0.0, label_cost=0.5)
            self.emit("expand_alpha", lam=0.0, label_cost=0.5, alpha=0)
        self.emit("set_labels", labels=np.zeros(n, np.int32))
        self.emit("energy", lam=0.0, label_cost=0.5)

    def h_masks_then_without(self):
        self.upload()
        self.emit("score_launch", T2=self.T2, has_compound=False, want_masks=True)
        self.emit("score_fetch", exponent=2, want_masks=True)
        self.emit("score_inliers", row=0)
        self.emit("score_launch", T2=self.T2, has_compound=False, want_masks=False)
        self.emit("score_fetch", exponent=2, want_masks=False)
        self.emit("score_fetch", exponent=1, want_masks=False)
        if self.may_refuse(2):
            self.emit("score_fetch", exponent=2, want_masks=True)
            self.emit("score_inliers", row=0)

    def h_new_points_same_n(self):
        """everything in use, then new points of the same n"""
        self.weights()
        self.preference()
        self.compound_update()
        self.labels()
        self.launch(masks=True)
        if self.mt != CM.NO_SOLVER_TYPE and self.m.n >= O.SAMPLE_SIZE[self.mt]:
            self.prosac_table()
        self.emit("score_set_global_n", n_total=50_000_000)
        round_type = self.name in ("sphere", "circle")
        if round_type:
            self.radius_range()
        self.new_points(same_n=True, name=self.name if round_type else None)
        if round_type:
            self.solve()
        if self.mt in CM.ACCUMULATOR_TYPES:
            self.launch()
            self.emit("score_accumulators")
        for _ in range(3):
            self.observe()

    def refused_radius_range(self):
        round_type = self.name in ("sphere", "circle")
        if not round_type and "sphere" in self.types and self.rng.random() < 0.5:
            self.new_points(same_n=True, name=self.pick(["sphere", "circle"]))
            round_type = True
        if round_type and self.m.oc.radius_range == (0.0, float("inf")):
            self.radius_range()
        self.emit("set_radius_range", rmin=float(self.pick([-1.0, 2.0, float("nan")])), rmax=1.0)
        if round_type:
            self.solve()

    # -- refusals: one documented, host-side PGX_ERR_INVALID, provoked singly by an existing test
    def refusal(self):
        """one refused call, drawn by the sentence it contradicts: every sentence available now is as likely as any other, and one
        this sequence has not contradicted yet comes first"""
        if "solver" not in self.drawn and self.mt != CM.NO_SOLVER_TYPE and "homography_sym" in self.types and self.rng.random() < 0.15:
            self.new_points(same_n=True, name="homography_sym")
        m = self.m
        menu = {}

        def add(tag, fn):
            menu.setdefault(tag, []).append(fn)
        fetch = lambda masks=False: self.emit("score_fetch", exponent=2, want_masks=masks)      # noqa: E731
        inliers = lambda: self.emit("score_inliers", row=0)                                     # noqa: E731
        add("points", self.refused_points)
        add("radius", self.refused_radius_range)
        if m.batch is not None:
            add("upload", lambda: (self.emit("score_upload", models=self.models[:0]), self.observe()))
        if m.launch is not None and m.batch is not None and not self.current():
            add("changed", fetch)
            if m.mask_rows is not None:
                add("changed rows", inliers)
        elif m.launch is not None and m.batch is not None:
            add("changed", lambda: (self.upload() if self.rng.random() < 0.5 else self.solve(), fetch()))
            if m.mask_rows is not None:
                add("changed rows", lambda: (self.upload() if self.rng.random() < 0.5 else self.solve(), inliers()))
        if m.batch is None:
            add("nothing", fetch)
        if m.mask_rows is None and (m.batch is None or (m.launch is not None and not m.launch["masks"])):
            add("no rows", inliers)
        if self.current() and not m.launch["masks"]:
            add("no masks", lambda: fetch(True))
        if self.mt == CM.NO_SOLVER_TYPE:
            add("solver", lambda: (self.emit("solve_minimal", samples=np.zeros((4, 2), np.int32)), self.observe()))
            add("solver", lambda: self.emit("solve_minimal_sampled", sampler="uniform", key=5, batch=1, S=64))
        elif m.n >= O.SAMPLE_SIZE[self.mt]:
            add("samples", lambda: (self.emit("solve_minimal", samples=self.samples(2)[:0]), self.observe()))
            add("prosac", lambda: self.emit("solve_minimal_sampled", sampler="prosac", key=5, batch=1, S=64 if self.m.prosac is None else len(self.m.prosac) + 1))
            if m.graph_n != m.n:
                add("napsac", lambda: self.emit("solve_minimal_sampled", sampler="napsac", key=5, batch=1, S=64))
        if m.graph_n != m.n:
            add("cut", lambda: self.emit("gc_labeling", model=self.models[0].copy(), T2=self.T2, lam=0.2))
        if m.oc.Dq is None:
            add("table", lambda: self.emit("greedy_labeling", label_cost=1.0))
            add("table", lambda: self.emit("energy", lam=0.0, label_cost=1.0))
        elif m.oc.labels is None or len(m.oc.labels) != m.dq_n:
            add("length", lambda: self.emit("energy", lam=0.0, label_cost=1.0))
            add("length", lambda: self.emit("expansion", lam=0.0, label_cost=1.0, max_cycles=1))
        elif m.labels_max >= m.L:
            add("range", lambda: self.emit("energy", lam=0.0, label_cost=1.0))
            add("range", lambda: self.emit("expand_alpha", lam=0.0, label_cost=1.0, alpha=0))
        else:
            add("alpha", lambda: self.emit("expand_alpha", lam=0.0, label_cost=1.0, alpha=int(self.pick([m.L, m.L + 3, -1]))))
            if m.graph_n != m.dq_n:
                add("lambda", lambda: self.emit("energy", lam=0.2, label_cost=1.0))
                add("lambda", lambda: self.emit("expansion", lam=0.2, label_cost=1.0, max_cycles=2))
                add("lambda", lambda: self.emit("expand_alpha", lam=0.2, label_cost=1.0, alpha=0))
            add("length", lambda: (self.emit("set_labels", labels=np.zeros(m.dq_n + 1, np.int32)), self.emit("energy", lam=0.0, label_cost=1.0)))
            add("range", lambda: (self.emit("set_labels", labels=np.full(m.dq_n, m.L, np.int32)), self.emit("expansion", lam=0.0, label_cost=1.0, max_cycles=1)))
        if m.oc.labels is None or len(m.oc.labels) != m.n:
            add("labels", lambda: self.emit("gram", kind=GRAM_AFFINE, sel=("label", 0), params=None, use_weights=False, wpow=2))
            add("labels", lambda: self.emit("residual_sums", models=np.ascontiguousarray(self.models[:2])))
            add("labels", lambda: self.emit("residual_sum", model=self.models[0].copy(), label=0))
            add("labels", lambda: self.emit("gram_labels", kind=GRAM_AFFINE, K=2, params=None, use_weights=False, wpow=2))
        if m.oc.labels is None:
            add("labels", lambda: self.emit("bucket", L=3))
            add("labels", lambda: self.emit("get_labels"))
        if m.weights is None:
            add("weights", lambda: self.emit("gram", kind=GRAM_AFFINE, sel=("index", self.index(10 if m.n >= 10 else 1)), params=None, use_weights=True, wpow=2))
        free = [s for s in (0, 1, 2, 5, 9) if s not in m.oc.slots]
        if free:
            add("slot", lambda: self.emit("get_preference", slot=int(free[0])))
            add("slot", lambda: self.emit("compound_update", slots=[int(free[-1])]))
        tags = sorted(menu)
        fresh = [t for t in tags if t not in self.drawn]
        rare = [t for t in (fresh or tags) if t in ("napsac", "solver", "lambda", "cut", "length", "table", "nothing", "changed rows", "no masks", "labels")]
        tag = self.pick(rare if rare and self.rng.random() < 0.7 else (fresh or tags))
        self.drawn.add(tag)
        self.pick(menu[tag])()

    def run(self):
        # a context outlives a sequence: what pgx_set_points leaves alone - the radius range, the graph - is set first
        self.emit("set_radius_range", rmin=0.0, rmax=float("inf"))
        self.new_points()
        self.graph_of_points()
        plain = [(self.score, 5), (self.upload, 2), (self.launch, 3), (self.fetch, 4), (self.inliers, 3), (self.accumulators, 3), (self.solve, 3),
                 (self.sampled, 5), (self.prosac_table, 1), (self.radius_range, 2), (self.compound, 2), (self.weights, 2), (self.preference, 3),
                 (self.get_preference, 2), (self.compound_update, 2), (self.pearl, 3), (self.inject, 2), (self.labels, 2), (self.energy, 3),
                 (self.expand_alpha, 3), (self.expansion, 4), (self.greedy, 2), (self.label_form, 9), (self.gram_index, 3), (self.gram_batch, 2),
                 (self.pnp_refine, 3), (self.eigh, 1), (self.epipolar, 3), (self.cut, 3), (self.graph_of_points, 2), (self.graph_read, 2),
                 (self.observe, 3), (self.new_points, 5), (self.h_identical_expansion, 2), (self.h_from_zeros_again, 2),
                 (self.h_masks_then_without, 2), (self.h_moves_wrote_nothing, 3), (self.h_new_points_same_n, 2)]
        w = np.array([x[1] for x in plain], dtype=np.float64)
        w /= w.sum()
        while len(self.ops) < OPS_PER_SEQUENCE:
            if self.rng.random() < P_REFUSED and self.may_refuse():
                self.refusal()
            else:
                plain[int(self.rng.choice(len(plain), p=w))][0]()
        return self.ops


def generate(seed, types=None):
    """the ops of sequence `seed`: a pure function of the seed (the true model decides what is valid; no device is asked).  types: the
    model types to draw, by name (default: all nine)"""
    return _Gen(seed, types).run()


SEEDS = (3, 6, 7, 9, 10, 11, 22, 24, 33)       # the committed sequences (tests/test_sequences_cpu.py holds what they must cover)
HOST_TYPES = ("homography", "pnp", "homography_sym")   # the types the host preprocessing (PGX_SETPOINTS_HOST=1) sorts like the device


def history_memo_restore():
    """The history behind the one bug the sequences found (docs/lab-notebook.md): an expansion from the uploaded zeros whose WHOLE
    first cycle is restored from the memo of the one before (same models, weights, graph) and that stops after that cycle runs no
    move, so nothing told labels_max what the restored labelling holds; a smaller table then passed the range check with labels
    beyond it resident.  Written out, because a seed only meets it when five draws fall together."""
    g = _Gen(0, types=("pnp",))
    g.emit("set_radius_range", rmin=0.0, rmax=float("inf"))
    g.idx = N_LIST.index(1025)
    g.new_points(same_n=True, name="pnp")
    g.ops, g.outs, g.refused = g.ops[:2], g.outs[:2], 0              # (without the refusal new_points may have drawn)
    g.m = ContextModel()
    for op in g.ops:
        g.m.step(op)
    g.emit("graph_build", points=g.pts, kind=2, radius=0.0, k=5)
    g.pearl(K=4, lam=0.1)
    g.emit("set_labels", labels=np.zeros(1025, np.int32))
    g.emit("expansion", lam=0.1, label_cost=3.0, max_cycles=1000)
    g.emit("get_labels")
    g.emit("set_labels", labels=np.zeros(1025, np.int32))
    g.pearl(K=4, lam=0.1)
    g.emit("expansion", lam=0.1, label_cost=3.0, max_cycles=1)       # every move of its only cycle comes from the memo
    g.emit("get_labels")
    assert int(g.m.oc.labels.max()) >= 2, "the labelling holds large labels"
    g.pearl(K=1, lam=0.1)                                            # two labels: the labels above are out of range now
    g.emit("energy", lam=0.0, label_cost=3.0)
    g.emit("expand_alpha", lam=0.0, label_cost=3.0, alpha=0)
    g.emit("expansion", lam=0.1, label_cost=3.0, max_cycles=1)
    assert [o[0] for o in g.outs[-3:]] == ["refused"] * 3
    g.emit("set_labels", labels=np.zeros(1025, np.int32))
    g.emit("expansion", lam=0.1, label_cost=3.0, max_cycles=1000)
    g.emit("get_labels")
    return g.ops


HISTORIES = {"memo-restore": history_memo_restore}


def sequence(which):
    """the ops of a committed seed or of a written-out history"""
    return HISTORIES[which]() if which in HISTORIES else generate(which)


# ---------------------------------------------------------------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------------------------------------------------------------
def _raw_gram(ctx, lib, kind, sel, params, use_weights, wpow):
    """pgx_gram with use_weights as given (Context.gram uploads the weights it is handed: the RESIDENT ones are under test here)"""
    q = lib.GRAM_Q.get(kind, lib.POINT_DIM[ctx.model_type] + 1)
    out = np.zeros(q * (q + 1) // 2)
    prm = None if params is None else np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    cnt, bad = C.c_int64(), C.c_int64()
    if sel[0] == "index":
        idx = np.ascontiguousarray(sel[1], dtype=np.int32)
        mode, iptr, m, label = 0, C.c_void_p(idx.ctypes.data) if idx.size else None, idx.size, 0
    else:
        mode, iptr, m, label = 1, None, 0, int(sel[1])
    ctx._ck(ctx._lib.pgx_gram(ctx._h, C.c_int(int(kind)), None if prm is None else C.c_void_p(prm.ctypes.data), C.c_int(0 if prm is None else prm.size),
                              C.c_int(mode), iptr, C.c_int64(m), C.c_int(label), C.c_int(1 if use_weights else 0), C.c_int(int(wpow)),
                              C.c_void_p(out.ctypes.data), C.byref(cnt), C.byref(bad)), "pgx_gram")
    return {"g_G": lib.tri_to_sym(out, q), "count": int(cnt.value), "bad": int(bad.value)}


def _raw_gram_labels(ctx, lib, kind, K, params, use_weights, wpow):
    q = lib.GRAM_Q.get(kind, lib.POINT_DIM[ctx.model_type] + 1)
    nv = q * (q + 1) // 2
    out, cnt, bad = np.zeros((K, nv)), np.zeros(K, np.int64), np.zeros(K, np.int64)
    prm = None if params is None else np.ascontiguousarray(params, dtype=np.float64).reshape(K, -1)
    ctx._ck(ctx._lib.pgx_gram_labels(ctx._h, C.c_int(int(kind)), None if prm is None else C.c_void_p(prm.ctypes.data),
                                     C.c_int(0 if prm is None else prm.shape[1]), C.c_int(int(K)), C.c_int(1 if use_weights else 0), C.c_int(int(wpow)),
                                     C.c_void_p(out.ctypes.data), C.c_void_p(cnt.ctypes.data), C.c_void_p(bad.ctypes.data)), "pgx_gram_labels")
    return {"g_G": [lib.tri_to_sym(out[k], q) for k in range(K)], "count": cnt, "bad": bad}


def _score_result(r, want_masks, exponent):
    return {"counts": r["counts"], "f_values": r["values"], "f_shared": r["shared"], "s_scores": (r["scores"], exponent),
            "masks": r["masks"] if want_masks else None}


def call(ctx, name, kw):
    """one op on a device context -> the result in the model's form; PgxError propagates"""
    from pyprogressivex import _lib
    if name == "set_points":
        mt, pts = kw["model_type"], kw["points"]
        if mt in _lib.POINT_DIM and pts.shape[0] > 0:
            return ctx.set_points(mt, pts)
        pts = np.ascontiguousarray(pts, dtype=np.float64)            # (Context.set_points indexes its tables with the type: the refusal is the library's)
        buf = pts if pts.size else np.zeros(8)
        return ctx._ck(ctx._lib.pgx_set_points(ctx._h, C.c_int(int(mt)), C.c_void_p(buf.ctypes.data), C.c_int64(pts.shape[0])), "pgx_set_points")
    if name in ("set_weights", "set_compound", "score_set_global_n", "score_upload", "score_launch", "sampler_prosac_set", "set_unary_q",
                "set_graph", "set_labels", "set_radius_range"):
        return getattr(ctx, name)(**kw)
    if name == "get_compound":
        return {"compound": ctx.get_compound()}
    if name == "score":
        return _score_result(ctx.score(**kw), kw["want_masks"], kw["exponent"])
    if name == "score_fetch":
        return _score_result(ctx.score_fetch(**kw), kw["want_masks"], kw["exponent"])
    if name == "score_inliers":
        return {"inliers": ctx.score_inliers(kw["row"])}
    if name == "score_accumulators":
        a = ctx.score_accumulators()
        out = {"acc_counts": a["counts"], "acc_values_q": a["values_q"]}
        if getattr(ctx, "_seq_has_compound", False):
            out["acc_shared_q"] = a["shared_q"]
        return out
    if name == "solve_minimal":
        return {"models": ctx.solve_minimal(kw["samples"])}
    if name == "solve_minimal_sampled":
        models, rows = ctx.solve_minimal_sampled(kw["key"], kw["batch"], kw["S"], fetch=True, fetch_samples=True, sampler=kw["sampler"])
        return {"samples": rows, "models": models}
    if name == "preference":
        r = ctx.preference(kw["model"], kw["T2"], kw["slot"], want_pref=True)
        return {"pref": r["pref"], "f_dot": r["dot"], "f_pref_sqnorm": r["pref_sqnorm"], "f_comp_sqnorm": r["comp_sqnorm"]}
    if name == "get_preference":
        return {"pref": ctx.get_preference(kw["slot"])}
    if name == "compound_update":
        return {"compound": ctx.compound_update(kw["slots"], want_compound=True)}
    if name == "pearl_unary":
        return {"table": ctx.pearl_unary(kw["models"] if len(kw["models"]) else None, kw["threshold"], kw["lam"], want_table=True)}
    if name == "residual_sum":
        return {"f_sum": ctx.residual_sum(kw["model"], kw["label"])}
    if name == "residual_sums":
        return {"f_sums": ctx.residual_sums(kw["models"])}
    if name == "bucket":
        ctx._nlabels = getattr(ctx, "_nlabels", 1)
        counts, order = ctx.bucket(kw["L"])
        return {"counts": counts, "order": order}
    if name == "epipolar_support":
        return {"support": np.array(ctx.epipolar_support(kw["F"], kw["T2"], kw["S2"]), dtype=np.int64)}
    if name == "gc_labeling":
        return {"flags": ctx.gc_labeling(kw["model"], kw["T2"], kw["lam"])}
    if name == "gc_inliers":
        return {"inliers": ctx.gc_inliers(kw["model"], kw["T2"], kw["lam"])}
    if name == "gram":
        return _raw_gram(ctx, _lib, **kw)
    if name == "gram_labels":
        return _raw_gram_labels(ctx, _lib, **kw)
    if name == "gram_batch":
        G, bad = ctx.gram_batch(kw["kind"], kw["index"], params=kw["params"], weights=kw["weights"], wpow=kw["wpow"])
        return {"g_G": list(G), "bad": bad.astype(np.int64)}
    if name == "pnp_refine_batch":
        P, ok = ctx.pnp_refine_batch(kw["inits"], kw["index"], iterations=kw["iterations"])
        return {"p_poses": (P, ok), "ok": ok}
    if name == "eigh_smallest_batch":
        vec, val = ctx.eigh_smallest_batch(kw["A"])
        return {"vec": vec, "val": val}
    if name == "graph_build":
        g = ctx.graph_build(kw["points"], kw["kind"], radius=kw["radius"], k=kw["k"])
        return {"off": g[0], "idx": g[1], "mult": g[2]}
    if name == "graph_fetch":
        g = ctx.graph_fetch()
        return {"off": g[0], "idx": g[1], "mult": g[2]}
    if name == "graph_size":
        return {"size": np.array(ctx.graph_size(), dtype=np.int64)}
    if name == "get_labels":
        ctx._nlabels = getattr(ctx, "_nlabels", 1)
        return {"labels": ctx.get_labels()}
    if name == "energy":
        eq, e = ctx.energy(kw["lam"], kw["label_cost"])
        return {"energy_q": eq, "energy": e}
    if name == "expand_alpha":
        return {"changed": ctx.expand_alpha(kw["lam"], kw["label_cost"], kw["alpha"])}
    if name == "expansion":
        eq, e, cyc = ctx.expansion(kw["lam"], kw["label_cost"], kw["max_cycles"])
        return {"energy_q": eq, "energy": e, "cycles": cyc}
    if name == "greedy_labeling":
        eq, e, opened = ctx.greedy_labeling(kw["label_cost"])
        return {"energy_q": eq, "energy": e, "opened": opened}
    raise KeyError(name)


def _invalid(err):
    return "failed (-1)" in str(err)


def attempt(ctx, op):
    """("ok", result) | ("refused", text) for PGX_ERR_INVALID | ("error", text) for every other failure: the caller stops there"""
    from pyprogressivex import _lib
    name, kw = op
    try:
        out = ("ok", call(ctx, name, kw))
    except _lib.PgxError as e:
        return ("refused" if _invalid(e) else "error", str(e))
    if name in ("score", "score_launch"):
        ctx._seq_has_compound = bool(kw["has_compound"])
    return out


def resident_state(model):
    """the ops that bring a fresh context to the resident state the model lists: radius range, graph, points, weights, compound, global
    n, PROSAC table, the table (made again by pearl_unary with the same models, or injected), labels, the batch and its launch"""
    m, ops = model, []
    ops.append(("set_radius_range", dict(rmin=m.oc.radius_range[0], rmax=m.oc.radius_range[1])))
    if m.oc.graph is not None:
        ops.append(("set_graph", dict(off=m.oc.graph[0], idx=m.oc.graph[1], mult=m.oc.graph[2])))
    if m.oc.pts is not None:
        ops.append(("set_points", dict(model_type=m.mt, points=m.oc.pts)))
        if m.weights is not None:
            ops.append(("set_weights", dict(weights=m.weights)))
        ops.append(("set_compound", dict(compound=m.oc.comp)))
        ops.append(("score_set_global_n", dict(n_total=m.global_n)))
        if m.prosac is not None:
            ops.append(("sampler_prosac_set", dict(subset_sizes=m.prosac)))
    if m.table is not None:
        ops.append(("pearl_unary", dict(models=m.table[1], threshold=m.table[2], lam=m.table[3])) if m.table[0] == "pearl"
                   else ("set_unary_q", dict(Dq=m.table[1])))
    if m.oc.labels is not None:
        ops.append(("set_labels", dict(labels=m.oc.labels)))
    if m.batch is not None:
        ops.append(("score_upload", dict(models=m.batch)))
        if m.launch is not None and m.launch["batch_id"] == m.batch_id:
            # a launch keeps what it computed: under the compound vector and the global n of ITS time, which may have changed since
            ops.append(("set_compound", dict(compound=m.launch["comp"])))
            ops.append(("score_set_global_n", dict(n_total=m.launch["global_n"])))
            ops.append(("score_launch", dict(T2=m.launch["T2"], has_compound=m.launch["has_compound"], want_masks=m.launch["masks"])))
            ops.append(("set_compound", dict(compound=m.oc.comp)))
            ops.append(("score_set_global_n", dict(n_total=m.global_n)))
    return ops


def same(a, b):
    """bitwise equality of nested results (NaN == NaN)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


STOPPED = []      # (sequence op index, text) of a device failure that was not PGX_ERR_INVALID: nothing runs in this process after it


def run(ctx, ops, checkpoints=MAX_CHECKPOINTS, fresh=None):
    """the calls on `ctx`, never retried.  Returns dict(outcomes, stopped, checkpoints): outcomes[i] = ("ok", result) | ("refused", text);
    stopped = (index, text) of a failure that is not PGX_ERR_INVALID - no call is made after it, on any context; checkpoints =
    [(index, equal)] - the accepted computing call at `index` repeated on a fresh context (fresh() makes one) that has seen only the
    resident state the model lists, compared bit for bit"""
    from pyprogressivex import _lib
    if STOPPED:
        raise RuntimeError(f"an earlier sequence stopped on a device failure, nothing runs after it: {STOPPED[0]}")
    fresh = fresh or (lambda: _lib.Context(0))
    model = ContextModel()
    outcomes, marks = [], []
    stride = max(1, sum(name in CHECKPOINTED for name, _ in ops) // max(1, checkpoints))
    seen = 0
    for i, op in enumerate(ops):
        name = op[0]
        before = resident_state(model) if checkpoints and name in CHECKPOINTED else None
        out = attempt(ctx, op)
        if out[0] == "error":
            STOPPED.append((i, out[1]))
            return dict(outcomes=outcomes, stopped=(i, out[1]), checkpoints=marks)
        outcomes.append(out)
        expect = model.step(op)
        if before is not None and out[0] == "ok" and expect[0] == "ok":
            seen += 1
            if seen % stride == 0 and len(marks) < checkpoints:
                got = [out[1]]
                if name in WRITERS:
                    got.append(attempt(ctx, ("get_labels", {})))
                with fresh() as other:
                    alone = []
                    for o in before + [op] + ([("get_labels", {})] if name in WRITERS else []):
                        r = attempt(other, o)
                        if r[0] == "error":
                            STOPPED.append((i, "fresh context: " + r[1]))
                            return dict(outcomes=outcomes, stopped=(i, "fresh context: " + r[1]), checkpoints=marks)
                        alone.append(r)
                ok = all(r[0] == "ok" for r in alone[:len(before)]) and same(got[0], alone[len(before)][1] if alone[len(before)][0] == "ok" else None)
                if name in WRITERS:
                    ok = ok and same(got[1], alone[-1])
                marks.append((i, bool(ok)))
    return dict(outcomes=outcomes, stopped=None, checkpoints=marks)


# ---------------------------------------------------------------------------------------------------------------------------------
# judge
# ---------------------------------------------------------------------------------------------------------------------------------
def _rel_ok(a, b):
    """tests/test_gpu_switches.py _rel <= REL, NaN == NaN and inf == inf"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    eq = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        close = np.abs(a - b) <= REL * np.maximum(1e-300, np.maximum(np.abs(a), np.abs(b)))
    return bool(np.all(eq | close))


def _close_ok(G, Gr):
    """tests/test_gpu_switches.py _close: 1e-9 of the matrix scale; a zero matrix (an empty selection) must come back as zeros"""
    G, Gr = np.asarray(G, dtype=np.float64), np.asarray(Gr, dtype=np.float64)
    if G.shape != Gr.shape:
        return False
    if not np.isfinite(Gr).all():
        return same(G, Gr)
    scale = float(np.abs(Gr).max()) if Gr.size else 0.0
    return bool(np.abs(G - Gr).max() <= REL * scale) if Gr.size else True


def compare(got, ref):
    """None, or what differs: keys f_ are floating sums (_rel), g_ Gram matrices (_close), s_ scores (the scale of _check_score),
    p_ refitted poses (1e-9 of max(1, |pose|), where the reference converged); everything else bit for bit"""
    if not isinstance(got, dict) or not isinstance(ref, dict):
        return None if same(got, ref) else "result"
    if got.keys() != ref.keys():
        return "fields"
    for k in ref:
        g, r = got[k], ref[k]
        if k.startswith("f_"):
            ok = _rel_ok(g, r)
        elif k.startswith("g_"):
            ok = _close_ok(g, r) if not isinstance(r, list) else len(g) == len(r) and all(_close_ok(x, y) for x, y in zip(g, r))
        elif k.startswith("s_"):
            (gs, _), (rs, e) = g, r
            scale = np.maximum(np.abs(ref["f_values"]), np.abs(ref["f_shared"]) ** e) + 1e-300
            ok = np.shape(gs) == np.shape(rs) and bool(np.all(np.abs(np.asarray(gs) - rs) / scale <= REL))
        elif k.startswith("p_"):
            (gp, gok), (rp, rok) = g, r
            ok = np.shape(gp) == np.shape(rp) and all(np.abs(gp[b] - rp[b]).max() <= REL * max(1.0, np.abs(rp[b]).max()) for b in range(len(rp)) if rok[b] and gok[b])
        else:
            ok = same(g, r)
        if not ok:
            return k
    return None


def judge(model, ops, outcomes):
    """replays the ops on `model` -> [(index, op name, what)]: accepted against refused, the refusal's class, the results.  `outcomes`
    come from a device (refusals carry pgx_last_error's text) or from another model (they carry the class)"""
    bad = []
    for i, (op, out) in enumerate(zip(ops, outcomes)):
        exp = model.step(op)
        if exp[0] != out[0]:
            bad.append((i, op[0], f"{out[0]} where the model says {exp[0]}" + (f" ({out[1]})" if out[0] == "refused" and isinstance(out[1], str) else "")
                        + (f" ({exp[1].__name__})" if exp[0] == "refused" else "")))
        elif exp[0] == "refused":
            hit = re.search(exp[1].fragment, out[1]) is not None if isinstance(out[1], str) else out[1] is exp[1]
            if not hit:
                bad.append((i, op[0], f"refused as {out[1] if isinstance(out[1], str) else out[1].__name__}, the model says {exp[1].__name__}"))
        else:
            what = compare(out[1], exp[1])
            if what is not None:
                bad.append((i, op[0], f"{what} differs"))
    if len(outcomes) < len(ops):
        bad.append((len(outcomes), ops[len(outcomes)][0], "the sequence stopped here"))
    return bad


def model_outcomes(ops, off=()):
    m = ContextModel(off=off)
    return [m.step(op) for op in ops]


def coverage(seeds):
    """(calls per op name, refusals per class, the n that were resident, refused share per sequence, identical expansions answered)"""
    per_op, per_ref, ns, share, identical = {k: 0 for k in OP_NAMES}, {c.__name__: 0 for c in CM.REFUSALS}, set(), {}, 0
    for seed in seeds:
        ops = generate(seed)
        outs = model_outcomes(ops)
        last = None                                                   # the last accepted expansion and whether a writer, a table or a graph came since
        for op, out in zip(ops, outs):
            per_op[op[0]] += 1
            if out[0] == "refused":
                per_ref[out[1].__name__] += 1
                continue
            if op[0] == "set_points":
                ns.add(op[1]["points"].shape[0])
            if op[0] == "expansion":
                key = CM._key(op[1])
                identical += last == key
                last = key
            elif op[0] in WRITERS + ("pearl_unary", "set_unary_q", "set_graph", "graph_build", "set_points"):
                last = None
        share[seed] = sum(o[0] == "refused" for o in outs) / len(ops)
    return per_op, per_ref, ns, share, identical


def soak(seed, sequences, verbose=False, ctx=None, checkpoints=MAX_CHECKPOINTS, seeds=None):
    """sequences seed * 1000 + k (or `seeds`) on one long-lived context: the number of disagreements with the model, unequal
    checkpoints included; a call that fails with anything but PGX_ERR_INVALID ends the soak at once and counts"""
    from pyprogressivex import _lib
    own = ctx is None
    ctx = _lib.Context(0) if own else ctx
    bad = calls = marks = 0
    t0 = time.time()
    try:
        for s in (seeds if seeds is not None else [seed * 1000 + k for k in range(sequences)]):
            ops = generate(s)
            res = run(ctx, ops, checkpoints=checkpoints)
            calls += len(res["outcomes"])
            marks += len(res["checkpoints"])
            found = judge(ContextModel(), ops, res["outcomes"]) + [(i, ops[i][0], "a fresh context gives other bits") for i, ok in res["checkpoints"] if not ok]
            for f in found:
                print("DISAGREEMENT", dict(sequence=s), *f, flush=True)
            bad += len(found)
            CM.clear_cache()
            if res["stopped"] is not None:
                print("STOPPED", dict(sequence=s, op=res["stopped"][0], name=ops[res["stopped"][0]][0]), res["stopped"][1], flush=True)
                bad += 1
                break
    finally:
        if own:
            ctx.close()
    if verbose:
        print(f"sequence soak done: seed {seed}, {sequences} sequences, {calls} calls, {marks} checkpoints, {bad} disagreements, {time.time() - t0:.0f} s")
    return bad


if __name__ == "__main__":
    sys.exit(1 if soak(int(sys.argv[1]), int(sys.argv[2]), verbose=True) else 0)
