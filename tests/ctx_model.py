"""ContextModel - the residency and refusal contract of include/pgx.h as a small executable model (tests/soak_sequences.py holds a
device context to it over random call sequences; tests/test_sequences_cpu.py checks the model and the sequences without a GPU).

TEST INFRASTRUCTURE, never imported by the product package.  The model holds an OracleContext by composition and keeps beside it
the state pgx.h describes and the oracle context has no notion of: the weights, the PROSAC table, the global n, the resident batch
and the launch that scored it, the mask rows, the largest label a writer may have left.  Every expected result is computed by
pgx_oracle; identical computations are answered from a cache, so replaying a sequence on a model with one rule switched off costs
almost nothing.

Every residency or refusal rule is one named entry of RULES; ContextModel(off={name}) behaves as if pgx.h did not state that rule.
A rule that no committed sequence can tell from its absence is not tested (tests/test_sequences_cpu.py asserts there is none).

NOT in the model, because the contract makes them invisible: the first-cycle memo and its snapshots, the column identities, the
skip rule and the identical-call shortcut of pgx_expansion ("results are bit-identical with and without the memo", pgx.h above
pgx_set_labels).  A call the shortcut answers must return what the oracle's expansion returns from the same labels - which is what
the model computes for every expansion.  That pgx_set_points ends the memo is therefore held by the device-side checks
(a fresh context must give the same bits), not by a rule here.
"""
import hashlib

import numpy as np

import pgx_oracle as O
from helpers import fixed_point_accumulators
from oracle_ctx import OracleContext

SAMPLERS = ("uniform", "napsac", "prosac")
NO_SOLVER_TYPE = 5                 # PGX_HOMOGRAPHY_SYM: 18-parameter models are generated on the host
ACCUMULATOR_TYPES = (2, 3, 4, 6, 8, 10)   # the types whose launches keep integer accumulators (test_point_sharded_accumulators_are_exact)


# ---- refusals: one class per contract sentence; `fragment` is matched (re.search) against pgx_last_error -------------------------
class Refusal(Exception):
    fragment = ""


class BadModelType(Refusal):
    fragment = r"pgx_set_points: bad model type"


class EmptyPoints(Refusal):
    fragment = r"pgx_set_points: empty input"


class NothingLaunched(Refusal):          # no batch is resident (pgx_set_points made "none" resident) or nothing was launched yet
    fragment = r"nothing launched"


class BatchChanged(Refusal):             # "the hypothesis batch (or the points) changed since the last launch"
    fragment = r"changed since the last launch"


class MasksNotRequested(Refusal):        # a mask fetch of a launch without masks
    fragment = r"masks were not requested at launch"


class NoMaskRows(Refusal):               # pgx_score_inliers: "the last launch that produced masks" has been ended
    fragment = r"the last launch produced no masks"


class EmptyBatch(Refusal):               # a refused upload / solve
    fragment = r"empty hypothesis batch|empty sample batch"


class NoSolver(Refusal):                 # "Other model types: PGX_ERR_INVALID"
    fragment = r"no device solver for model type"


class TableNotSet(Refusal):
    fragment = r"unary table not set"


class LabelsNotSet(Refusal):             # no labels, or not of the length the call needs
    fragment = r"labels not set"


class LabelOutOfRange(Refusal):
    fragment = r"label \d+ out of range \(the unary table has \d+ labels\)"


class AlphaOutOfRange(Refusal):
    fragment = r"alpha -?\d+ out of range"


class GraphForLambda(Refusal):
    fragment = r"lambda > 0 but no graph set|lambda > 0 needs a graph over"


class GraphForNapsac(Refusal):
    fragment = r"NAPSAC needs the neighbourhood graph of the resident points"


class GraphForCut(Refusal):
    fragment = r"pgx_gc_labeling: needs a neighbourhood graph over"


class NoWeights(Refusal):
    fragment = r"use_weights set but no weights are resident"


class NoProsacTable(Refusal):            # missing, too short, or of other points
    fragment = r"PROSAC needs pgx_sampler_prosac_set for the resident points"


class EmptySlot(Refusal):
    fragment = r"slot \d+ is empty|slot \d+ holds no preference vector"


class BadRadiusRange(Refusal):
    fragment = r"pgx_set_radius_range: need 0 <= rmin <= rmax"


class Undrawn(Refusal):
    """a refusal the generator never draws (not documented in pgx.h, or not provoked singly by an existing test): the true model
    raising it while a sequence is generated is a bug of the generator"""
    fragment = r"$^"


REFUSALS = [BadModelType, EmptyPoints, NothingLaunched, BatchChanged, MasksNotRequested, NoMaskRows, EmptyBatch, NoSolver, TableNotSet,
            LabelsNotSet, LabelOutOfRange, AlphaOutOfRange, GraphForLambda, GraphForNapsac, GraphForCut, NoWeights, NoProsacTable,
            EmptySlot, BadRadiusRange]

# ---- the rules: name -> the sentence of include/pgx.h (or of the error text) it restates ------------------------------------------
RULES = {
    # pgx_set_points ends ...
    "points_end_unary": "pgx_set_points: the unary table belongs to a point set (dq_n = 0: 'unary table not set')",
    "points_end_labels": "pgx_set_points: the labels belong to a point set ('labels not set')",
    "points_end_weights": "pgx.h pgx_set_weights: 'pgx_set_points invalidates them'",
    "points_end_prosac": "pgx.h pgx_sampler_prosac_set: 'pgx_set_points invalidates the table'",
    "points_end_slots": "pgx_set_points releases every preference slot ('slot is empty')",
    "points_end_global_n": "pgx.h pgx_score_set_global_n: the scale of a sharded job belongs to that job's point set",
    "points_end_batch": "pgx.h above pgx_score_fetch: 'pgx_set_points make[s] another batch (or none) resident'",
    "points_end_mask_rows": "pgx.h pgx_score_inliers: 'pgx_set_points ends that launch'",
    "points_zero_compound": "pgx_set_points zeroes the compound vector",
    "points_keep_graph": "pgx_set_points leaves the neighbourhood graph alone",
    "points_keep_radius_range": "pgx.h pgx_set_radius_range: 'context state', not the point set's",
    "refused_points_change_nothing": "a refused pgx_set_points (bad type, n <= 0) changes nothing",
    # results belong to a batch
    "fetch_refused_after_new_batch": "pgx.h: pgx_score_fetch is refused after an upload or a solve, until the next launch",
    "inliers_refused_after_new_batch": "pgx.h: pgx_score_inliers is refused after 'a new batch'",
    "mask_fetch_needs_masks": "pgx_score_fetch: 'masks were not requested at launch'",
    "launch_without_masks_ends_mask_rows": "pgx.h pgx_score_inliers: 'a later launch without masks ... ends that launch'",
    "refused_upload_keeps_batch": "pgx.h: 'a refused or failed upload / solve changes nothing: the previous batch stays resident and its launch fetchable'",
    "launch_fetchable_twice": "one launch can be fetched twice",
    # preconditions
    "labels_of_table_length": "pgx_energy / pgx_expansion / pgx_expand_alpha: labels of the unary table's length",
    "labels_below_L": "label out of range (the unary table has L labels): the labels pgx_set_labels uploaded",
    "moves_raise_labels_max": "... and the labels moves may have written before a smaller table arrived",
    "alpha_in_range": "pgx_expand_alpha: alpha out of range",
    "graph_for_lambda": "lambda > 0 needs a graph over exactly the table's n sites",
    "graph_for_napsac": "the NAPSAC sampler needs the neighbourhood graph of the resident points",
    "graph_for_cut": "pgx.h pgx_gc_labeling: 'needs pgx_set_points + a graph over the points'",
    "label_forms_need_labels": "'labels not set' for the label forms: pgx_gram, pgx_gram_labels, pgx_residual_sum(s), pgx_bucket",
    "use_weights_needs_weights": "use_weights set but no weights are resident for the current points",
    "prosac_needs_table": "PROSAC needs a table of pgx_sampler_prosac_set with at least S entries",
    "empty_slot_refused": "pgx_get_preference / pgx_compound_update: an empty slot",
    "bad_radius_range_refused": "pgx.h pgx_set_radius_range: 'NaN, rmin < 0 or rmax < rmin: PGX_ERR_INVALID'",
    "refused_radius_range_keeps_old": "... which leaves the old range in place",
    "no_solver_for_18_parameters": "pgx.h pgx_solve_minimal: 'Other model types: PGX_ERR_INVALID'",
    # label writers
    "set_labels_writes": "pgx_set_labels uploads the labelling",
    "expand_alpha_writes": "pgx_expand_alpha writes the labelling",
    "expansion_writes": "pgx_expansion writes the labelling",
    "greedy_writes": "pgx.h pgx_greedy_labeling: 'the resident labelling is OVERWRITTEN' (and covers the table's sites)",
    "cut_keeps_pearl_state": "pgx_gc_labeling keeps the PEARL state (its cut is not a labelling)",
}


# ---- cached oracle calls ---------------------------------------------------------------------------------------------------------
_CACHE = {}


def _key(x):
    if isinstance(x, np.ndarray):
        return (x.shape, x.dtype.str, hashlib.blake2b(np.ascontiguousarray(x).tobytes(), digest_size=16).digest())
    if isinstance(x, (tuple, list)):
        return tuple(_key(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, _key(v)) for k, v in sorted(x.items()))
    return repr(x)


def cached(fn, *args, **kw):
    key = (fn.__module__, fn.__name__, _key(args), _key(kw))
    if key not in _CACHE:
        _CACHE[key] = fn(*args, **kw)
    return _CACHE[key]


def clear_cache():
    _CACHE.clear()


def _copy(r):
    if isinstance(r, dict):
        return {k: _copy(v) for k, v in r.items()}
    if isinstance(r, (tuple, list)):
        return type(r)(_copy(v) for v in r)
    return r.copy() if isinstance(r, np.ndarray) else r


EMPTY_GRAPH = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1, np.int32))


class ContextModel:
    def __init__(self, off=()):
        self.off = frozenset(off)
        assert self.off <= set(RULES), self.off - set(RULES)
        self.oc = OracleContext()
        self.oc.pts = None
        self.weights = None
        self.prosac = None
        self.global_n = 0
        self.batch = None          # the resident hypothesis batch [M, P]
        self.batch_id = 0          # bumped by every event that makes another batch resident
        self.launch = None         # dict(batch_id, masks, has_compound, table) of the last launch
        self.mask_rows = None      # dict(batch_id, masks) of the last launch that produced masks, until something ends it
        self.fetched = False
        self.labels_max = 0
        self.table = None          # how the resident table was made: ("pearl", models, thr, lam) | ("inject", Dq)

    # ---- plumbing
    def on(self, rule):
        assert rule in RULES, rule
        return rule not in self.off

    def step(self, op):
        """op = (name, kwargs) -> ("ok", result) | ("refused", class).  A model with a rule switched off may reach states the
        contract excludes (a labelling of another point set, say): whatever then breaks inside the oracle is a result like any other"""
        name, kw = op
        try:
            return ("ok", _copy(getattr(self, "op_" + name)(**kw)))
        except Refusal as r:
            return ("refused", type(r))
        except Exception as e:               # noqa: BLE001
            if not self.off:
                raise
            return ("ok", {"undefined": repr(e)[:80]})

    @property
    def n(self):
        return self.oc.n

    @property
    def mt(self):
        return self.oc.model_type

    @property
    def L(self):
        return 0 if self.oc.Dq is None else self.oc.Dq.shape[1]

    @property
    def dq_n(self):
        return 0 if self.oc.Dq is None else self.oc.Dq.shape[0]

    @property
    def graph_n(self):
        return 0 if self.oc.graph is None else len(self.oc.graph[0]) - 1

    def _need_points(self):
        if self.oc.pts is None:
            raise Undrawn("points not set")

    @staticmethod
    def _defined(ok, what):
        """the oracle's C code reads what it is handed: a state the contract excludes (reachable only with a rule switched off) is
        stopped here and becomes the result "undefined" (step)"""
        if not ok:
            raise RuntimeError("undefined: " + what)

    # ---- points and what belongs to them
    def _points_end(self):
        if self.on("points_end_unary"):
            self.oc.Dq, self.table = None, None
        if self.on("points_end_labels"):
            self.oc.labels, self.labels_max = None, 0
        if self.on("points_end_weights"):
            self.weights = None
        if self.on("points_end_prosac"):
            self.prosac = None
        if self.on("points_end_slots"):
            self.oc.slots = {}
        if self.on("points_end_global_n"):
            self.global_n = 0
        if self.on("points_end_batch"):
            self.batch, self.launch = None, None
            self.batch_id += 1
        if self.on("points_end_mask_rows"):
            self.mask_rows = None
        if not self.on("points_keep_graph"):
            self.oc.graph = None
        if not self.on("points_keep_radius_range"):
            self.oc.radius_range = (0.0, float("inf"))

    def op_set_points(self, model_type, points):
        if model_type not in O.POINT_DIM or points.shape[0] <= 0:
            if not self.on("refused_points_change_nothing"):
                self._points_end()
            raise BadModelType() if model_type not in O.POINT_DIM else EmptyPoints()
        old = self.oc.comp
        self._points_end()
        self.oc.pts = np.ascontiguousarray(points, dtype=np.float64)
        self.oc.model_type, self.oc.n = model_type, points.shape[0]
        self.oc.comp = np.zeros(self.n) if self.on("points_zero_compound") or old is None else old
        return None

    def op_set_weights(self, weights):
        self._need_points()
        self.weights = None if weights is None else weights.copy()

    def op_set_compound(self, compound):
        self._need_points()
        self.oc.set_compound(compound)

    def op_get_compound(self):
        self._need_points()
        return {"compound": self.oc.get_compound()}

    def op_set_radius_range(self, rmin, rmax):
        if not (rmin >= 0.0 and rmax >= rmin):
            if not self.on("refused_radius_range_keeps_old"):
                self.oc.radius_range = (0.0, float("inf"))
            if self.on("bad_radius_range_refused"):
                raise BadRadiusRange()
            return None
        self.oc.radius_range = (float(rmin), float(rmax))

    def op_score_set_global_n(self, n_total):
        self.global_n = int(n_total)

    # ---- the batch and its launch
    def _new_batch(self, models):
        self.batch = np.ascontiguousarray(models, dtype=np.float64).copy()
        self.batch_id += 1

    def _refused_upload(self, refusal):
        if not self.on("refused_upload_keeps_batch"):
            self.batch_id += 1
        raise refusal

    def op_score_upload(self, models):
        self._need_points()
        if models.shape[0] <= 0:
            self._refused_upload(EmptyBatch())
        self._new_batch(models)

    def op_score_launch(self, T2, has_compound, want_masks):
        self._need_points()
        if self.batch is None:
            raise Undrawn("no hypotheses uploaded")
        self._defined(len(self.oc.comp) == self.n and self.batch.shape[1] == O.PARAM_DIM[self.mt], "compound / batch of other points")
        table = cached(O.score, self.mt, self.oc.pts, self.batch, T2, compound=self.oc.comp, has_compound=bool(has_compound), exponent=2,
                       want_masks=True)
        acc = None
        if self.mt in ACCUMULATOR_TYPES:
            acc = cached(fixed_point_accumulators, O, self.mt, self.oc.pts, self.batch, T2, comp=self.oc.comp if has_compound else None,
                         n_total=max(self.global_n, self.n))
        self.launch = dict(batch_id=self.batch_id, T2=float(T2), masks=bool(want_masks), has_compound=bool(has_compound), table=table, acc=acc,
                           comp=self.oc.comp.copy(), global_n=self.global_n)      # (what the launch read: a checkpoint makes it again)
        self.fetched = False
        if want_masks:
            self.mask_rows = dict(batch_id=self.batch_id, masks=table["masks"])
        elif self.on("launch_without_masks_ends_mask_rows"):
            self.mask_rows = None

    def op_score_fetch(self, exponent, want_masks):
        if self.batch is not None and self.launch is None:
            raise Undrawn("a launch of an earlier history may be on record: 'nothing launched' or 'changed'")
        if self.batch is None or (self.fetched and not self.on("launch_fetchable_twice")):
            raise NothingLaunched()
        if self.on("fetch_refused_after_new_batch") and self.launch["batch_id"] != self.batch_id:
            raise BatchChanged()
        if want_masks and not self.launch["masks"] and self.on("mask_fetch_needs_masks"):
            raise MasksNotRequested()
        self.fetched = True
        t = self.launch["table"]
        scores = t["values"] - np.power(t["shared"], float(exponent)) if self.launch["has_compound"] else t["values"].copy()
        return {"counts": t["counts"], "f_values": t["values"], "f_shared": t["shared"], "s_scores": (scores, exponent),
                "masks": t["masks"] if want_masks else None}

    def op_score(self, models, T2, has_compound, exponent, want_masks):
        self.op_score_upload(models)
        self.op_score_launch(T2, has_compound, want_masks)
        return self.op_score_fetch(exponent, want_masks)

    def op_score_inliers(self, row):
        if self.mask_rows is None:
            if self.batch is not None and (self.launch is None or self.launch["masks"]):
                raise Undrawn("mask rows of an earlier history may be on record")
            raise NoMaskRows()
        if self.on("inliers_refused_after_new_batch") and self.mask_rows["batch_id"] != self.batch_id:
            raise BatchChanged()
        m = self.mask_rows["masks"]
        if not 0 <= row < m.shape[0]:
            raise Undrawn("row")
        bits = np.unpackbits(m[row].view(np.uint8), bitorder="little")[:self.n]
        return {"inliers": np.flatnonzero(bits).astype(np.int64)}

    def op_score_accumulators(self):
        if self.launch is None or self.launch["batch_id"] != self.batch_id or self.launch["acc"] is None or self.batch is None:
            raise Undrawn("accumulators")
        a = self.launch["acc"]
        out = {"acc_counts": a["counts"].astype(np.uint64), "acc_values_q": a["values_q"].astype(np.uint64)}
        if self.launch["has_compound"]:
            out["acc_shared_q"] = a["shared_q"].astype(np.uint64)
        return out

    # ---- minimal solvers
    def op_solve_minimal(self, samples):
        self._need_points()
        if samples.shape[0] <= 0:
            self._refused_upload(EmptyBatch())
        if self.mt == NO_SOLVER_TYPE and self.on("no_solver_for_18_parameters"):
            self._refused_upload(NoSolver())
        models = cached(O.solve_minimal, self.mt, self.oc.pts, samples, radius_range=self.oc.radius_range)
        self._new_batch(models)
        return {"models": models}

    def op_sampler_prosac_set(self, subset_sizes):
        self._need_points()
        self.prosac = subset_sizes.copy()

    def op_solve_minimal_sampled(self, sampler, key, batch, S):
        n, mt = self.n, self.mt
        if sampler == "prosac" and self.on("prosac_needs_table") and (self.prosac is None or len(self.prosac) < S):
            self._refused_upload(NoProsacTable())
        if sampler == "napsac" and self.on("graph_for_napsac") and (self.graph_n != n or len(self.oc.graph[1]) == 0):
            self._refused_upload(GraphForNapsac())
        self._need_points()
        if S <= 0:
            self._refused_upload(EmptyBatch())
        if mt == NO_SOLVER_TYPE and self.on("no_solver_for_18_parameters"):
            self._refused_upload(NoSolver())
        self._defined(mt in O.SAMPLE_SIZE, "no solver")
        m = O.SAMPLE_SIZE[mt]
        if n < m:
            raise Undrawn("fewer points than the minimal sample")
        if sampler == "uniform":
            rows = cached(O.sample_uniform, key, batch, 0, S, n, m)
        elif sampler == "napsac":
            self._defined(self.graph_n == n and len(self.oc.graph[1]) > 0, "graph of other points")
            rows = cached(O.sample_napsac, key, batch, 0, S, n, self.oc.graph[0], self.oc.graph[1], m)
        else:
            self._defined(self.prosac is not None and len(self.prosac) >= S and int(self.prosac.max()) <= n, "table of other points")
            rows = cached(O.sample_prosac, key, batch, 0, S, n, self.prosac[:S], m)
        absent = rows[:, 0] < 0                                   # "the row -1 .. -1 and a NaN model (the iteration is spent)"
        models = cached(O.solve_minimal, mt, self.oc.pts, np.where(absent[:, None], 0, rows).astype(np.int32),
                        radius_range=self.oc.radius_range).copy()
        slots = models.shape[0] // S
        models.reshape(S, slots, -1)[absent] = np.nan
        self._new_batch(models)
        return {"samples": rows, "models": models}

    # ---- pointwise
    def op_preference(self, model, T2, slot):
        self._need_points()
        p = cached(O.preference, self.mt, self.oc.pts, model, T2)
        self._defined(len(self.oc.comp) == self.n, "compound of other points")
        self.oc.slots[slot] = p
        d, a, b = O.tanimoto_terms(p, self.oc.comp)
        return {"pref": p, "f_dot": d, "f_pref_sqnorm": a, "f_comp_sqnorm": b}

    def op_get_preference(self, slot):
        if slot not in self.oc.slots:
            if self.on("empty_slot_refused"):
                raise EmptySlot()
            return {"pref": np.zeros(self.n)}
        return {"pref": self.oc.slots[slot]}

    def op_compound_update(self, slots):
        self._need_points()
        if any(s not in self.oc.slots for s in slots):
            if self.on("empty_slot_refused"):
                raise EmptySlot()
            slots = [s for s in slots if s in self.oc.slots]
        self._defined(all(len(self.oc.slots[s]) == self.n for s in slots), "slots of other points")
        return {"compound": self.oc.compound_update(slots, want_compound=True)}

    def op_pearl_unary(self, models, threshold, lam):
        self._need_points()
        Dq = cached(O.unary_q, self.mt, self.oc.pts, models, threshold, lam)
        self.oc.Dq = Dq
        self.table = ("pearl", models, threshold, lam)
        return {"table": Dq}

    def op_set_unary_q(self, Dq):
        self.oc.Dq = Dq
        self.table = ("inject", Dq)

    def _labels_of_points(self):
        if self.on("label_forms_need_labels") and (self.oc.labels is None or len(self.oc.labels) != self.n):
            raise LabelsNotSet()
        self._defined(self.oc.labels is not None and len(self.oc.labels) == self.n, "labels of other points")

    def op_residual_sum(self, model, label):
        self._need_points()
        self._labels_of_points()
        return {"f_sum": O.residual_sum(self.mt, self.oc.pts, model, self.oc.labels, label)}

    def op_residual_sums(self, models):
        self._need_points()
        self._labels_of_points()
        return {"f_sums": np.array([O.residual_sum(self.mt, self.oc.pts, m, self.oc.labels, k) for k, m in enumerate(models)])}

    def op_bucket(self, L):
        if self.on("label_forms_need_labels") and self.oc.labels is None:
            raise LabelsNotSet()
        self._defined(self.oc.labels is not None and int(self.oc.labels.max()) < L, "no labels")
        counts, order = O.bucket(self.oc.labels, L)
        return {"counts": counts, "order": order}

    def op_epipolar_support(self, F, T2, S2):
        self._need_points()
        a, b = O.epipolar_support(self.oc.pts, F, T2, S2)
        return {"support": np.array([a, b], dtype=np.int64)}

    def _cut(self, model, T2, lam):
        self._need_points()
        if self.on("graph_for_cut") and self.graph_n != self.n:
            raise GraphForCut()
        self._defined(self.graph_n == self.n, "graph of other points")
        flags = cached(O.gc_labeling, self.mt, self.oc.pts, model, T2, lam, self.oc.graph)
        if not self.on("cut_keeps_pearl_state"):
            self.oc.labels = flags.astype(np.int32)
            self.labels_max = 1
        return flags

    def op_gc_labeling(self, model, T2, lam):
        return {"flags": self._cut(model, T2, lam)}

    def op_gc_inliers(self, model, T2, lam):
        return {"inliers": np.flatnonzero(self._cut(model, T2, lam) != 0).astype(np.int64)}

    # ---- fits
    def _w(self, use_weights):
        if not use_weights:
            return None
        if self.weights is None:
            if self.on("use_weights_needs_weights"):
                raise NoWeights()
            return np.ones(self.n)
        return self.weights

    def op_gram(self, kind, sel, params, use_weights, wpow):
        self._need_points()
        if sel[0] == "label":
            self._labels_of_points()
            index = np.flatnonzero(self.oc.labels == int(sel[1]))
        else:
            index = np.asarray(sel[1], dtype=np.int64)
        G, cnt, bad = O.gram(kind, self.oc.pts, index, params=params, weights=self._w(use_weights), wpow=wpow)
        return {"g_G": G, "count": int(cnt), "bad": int(bad)}

    def op_gram_labels(self, kind, K, params, use_weights, wpow):
        self._need_points()
        self._labels_of_points()
        w = self._w(use_weights)
        res = [O.gram(kind, self.oc.pts, np.flatnonzero(self.oc.labels == k), params=None if params is None else params[k], weights=w, wpow=wpow)
               for k in range(K)]
        return {"g_G": [r[0] for r in res], "count": np.array([r[1] for r in res], np.int64), "bad": np.array([r[2] for r in res], np.int64)}

    def op_gram_batch(self, kind, index, params, weights, wpow):
        self._need_points()
        G, bad = self.oc.gram_batch(kind, index, params=params, weights=weights, wpow=wpow)
        return {"g_G": list(G), "bad": bad.astype(np.int64)}

    def op_pnp_refine_batch(self, inits, index, iterations):
        self._need_points()
        P, ok = self.oc.pnp_refine_batch(inits, index, iterations=iterations)
        return {"p_poses": (P, ok), "ok": ok}

    def op_eigh_smallest_batch(self, A):
        vec, val, _ = cached(O.eigh_smallest, A)
        return {"vec": vec, "val": val}

    # ---- graph
    def op_graph_build(self, points, kind, radius, k):
        self.oc.graph = cached(O.graph_build, points, kind, radius=radius, k=k)
        return {"off": self.oc.graph[0], "idx": self.oc.graph[1], "mult": self.oc.graph[2]}

    def op_set_graph(self, off, idx, mult):
        self.oc.set_graph(off, idx, mult)

    def op_graph_fetch(self):
        if self.oc.graph is None:
            raise Undrawn("no graph is resident")
        return {"off": self.oc.graph[0], "idx": self.oc.graph[1], "mult": self.oc.graph[2]}

    def op_graph_size(self):
        return {"size": np.array([self.graph_n, 0 if self.oc.graph is None else len(self.oc.graph[1])], dtype=np.int64)}

    # ---- labelling
    def op_set_labels(self, labels):
        if self.on("set_labels_writes"):
            self.oc.labels = labels.astype(np.int32).copy()
            self.labels_max = int(labels.max())

    def op_get_labels(self):
        if self.oc.labels is None:
            raise LabelsNotSet()
        return {"labels": self.oc.labels}

    def _resident_problem(self, lam, alpha=None):
        """what pgx_energy, pgx_expand_alpha and pgx_expansion ask of the resident problem, in the library's order"""
        if self.oc.Dq is None:
            raise TableNotSet()
        if self.on("labels_of_table_length") and (self.oc.labels is None or len(self.oc.labels) != self.dq_n):
            raise LabelsNotSet()
        seen = self.labels_max if self.on("moves_raise_labels_max") or self.oc.labels is None else int(self.oc.labels.max())
        if self.on("labels_below_L") and seen >= self.L:
            raise LabelOutOfRange()
        if alpha is not None and self.on("alpha_in_range") and not 0 <= alpha < self.L:
            raise AlphaOutOfRange()
        if O.quantize_lambda(lam) > 0 and self.on("graph_for_lambda") and self.graph_n != self.dq_n:
            raise GraphForLambda()
        lab = self.oc.labels
        self._defined(lab is not None and len(lab) == self.dq_n and int(lab.max()) < self.L and (alpha is None or 0 <= alpha < self.L)
                      and (O.quantize_lambda(lam) <= 0 or self.graph_n == self.dq_n), "labels, alpha or graph of another problem")

    def _graph_arg(self, lam):
        if O.quantize_lambda(lam) > 0 and self.oc.graph is not None and len(self.oc.graph[1]) > 0:
            return self.oc.graph
        return (np.zeros(self.dq_n + 1, np.int32), np.zeros(1, np.int32), np.ones(1, np.int32))

    def op_energy(self, lam, label_cost):
        self._resident_problem(lam)
        e = cached(O.energy, self.oc.Dq, self._graph_arg(lam), O.quantize_lambda(lam), O.quantize(label_cost), self.oc.labels.copy())
        return {"energy_q": int(e), "energy": e / 2.0 ** 32}

    def op_expand_alpha(self, lam, label_cost, alpha):
        self._resident_problem(lam, alpha)
        labels, ch, _ = cached(O.expand_alpha, self.oc.Dq, self._graph_arg(lam), O.quantize_lambda(lam), O.quantize(label_cost), alpha,
                               self.oc.labels.copy())
        if self.on("expand_alpha_writes"):
            self.oc.labels = labels
        self.labels_max = max(self.labels_max, alpha)
        return {"changed": int(ch)}

    def op_expansion(self, lam, label_cost, max_cycles):
        self._resident_problem(lam)
        labels, e, cyc = cached(O.expansion, self.oc.Dq, self._graph_arg(lam), O.quantize_lambda(lam), O.quantize(label_cost), self.oc.labels.copy(),
                                max_cycles)
        if self.on("expansion_writes"):
            self.oc.labels = labels
        self.labels_max = max(self.labels_max, self.L - 1)
        return {"energy_q": int(e), "energy": e / 2.0 ** 32, "cycles": int(cyc)}

    def op_greedy_labeling(self, label_cost):
        if self.oc.Dq is None:
            raise TableNotSet()
        labels, e, opened = cached(O.greedy_labeling, self.oc.Dq, O.quantize(label_cost))
        if self.on("greedy_writes"):
            self.oc.labels = labels
        self.labels_max = self.L - 1
        return {"energy_q": int(e), "energy": e / 2.0 ** 32, "opened": int(opened)}
