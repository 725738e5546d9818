"""splitComponents without a GPU: the public function's signature and argument checks, the ABI entry, _components.regroup against the
restatement of its definition (components_model.py), and the find / link statements of csrc/components_uf.h - the lines the kernels of
components.hip run - on std::atomic (tests/emu/components_driver.cpp): arc by arc in many orders, and under eight threads, against the
breadth-first search of components_model.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import components_model as CM
import pyprogressivex as px
from pyprogressivex import _components, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pgx.h")


# ---- the public function ----------------------------------------------------------------------------------------------------------------
def test_split_components_is_exported_with_its_signature():
    assert "splitComponents" in px.__all__
    sig = inspect.signature(px.splitComponents)
    assert list(sig.parameters) == ["points", "labels", "model_number", "k", "radius", "minimum_point_number", "keep"]
    assert [p.default for p in sig.parameters.values()][3:] == [16, None, 10, "all"]
    doc = " ".join(px.splitComponents.__doc__.split())
    for phrase in ("largest gap that still counts as one surface", "joins stragglers over any distance", "k <= 16",
                   "changes nothing about how the find* calls score", "planes[parent]"):
        assert phrase in doc, phrase


POINTS = np.arange(30.0).reshape(10, 3)
LABELS = np.zeros(10, dtype=np.int32)


@pytest.mark.parametrize("args, kw, match", [
    ((np.zeros((10, 4)), LABELS, 1), {}, r"points should be an array with dims \[n,2\] or \[n,3\]"),
    ((np.zeros(10), LABELS, 1), {}, "points should be"),
    ((np.zeros((2, 5, 3)), LABELS, 1), {}, "points should be"),
    ((POINTS, np.zeros(9, dtype=np.int32), 1), {}, "labels should be an array with dims"),
    ((POINTS, np.zeros((10, 1), dtype=np.int32), 1), {}, "labels should be an array with dims"),
    ((POINTS, np.zeros(10), 1), {}, "labels should be integers"),
    ((POINTS, np.zeros(10, dtype=bool), 1), {}, "labels should be integers"),
    ((POINTS, LABELS, -1), {}, "model_number should be"),
    ((POINTS, LABELS, 1.5), {}, "model_number should be"),
    ((POINTS, LABELS, 1), dict(k=1), "k should be"),
    ((POINTS, LABELS, 1), dict(k=0), "k should be"),
    ((POINTS, LABELS, 1), dict(k=2.5), "k should be"),
    ((POINTS, LABELS, 1), dict(k=True), "k should be"),
    ((POINTS, LABELS, 1), dict(k=None), "k or radius"),
    ((POINTS, LABELS, 1), dict(radius=0.0), "radius should be"),
    ((POINTS, LABELS, 1), dict(radius=-1.0), "radius should be"),
    ((POINTS, LABELS, 1), dict(radius=float("nan")), "radius should be"),
    ((POINTS, LABELS, 1), dict(radius="far"), "radius should be"),
    ((POINTS, LABELS, 1), dict(minimum_point_number=0), "minimum_point_number should be"),
    ((POINTS, LABELS, 1), dict(minimum_point_number=2.0), "minimum_point_number should be"),
    ((POINTS, LABELS, 1), dict(keep="some"), 'keep should be "all" or "largest"'),
    ((POINTS, LABELS, 1), dict(keep=None), "keep should be"),
])
def test_split_components_rejects_bad_arguments_before_it_touches_the_context(args, kw, match, monkeypatch):
    from pyprogressivex import _api

    def no_context():
        raise AssertionError("the context was touched before the arguments were checked")
    monkeypatch.setattr(_api, "_context", no_context)
    with pytest.raises(ValueError, match=match):
        px.splitComponents(*args, **kw)


def test_the_argument_sentences_are_those_of_estimate_normals(monkeypatch):
    from pyprogressivex import _api
    monkeypatch.setattr(_api, "_context", lambda: pytest.fail("the context was touched"))
    for kw in (dict(k=1), dict(k=None), dict(radius=0.0), dict(radius="far")):
        with pytest.raises(ValueError) as a:
            px.estimateNormals(POINTS, **kw)
        with pytest.raises(ValueError) as b:
            px.splitComponents(POINTS, LABELS, 1, **kw)
        assert str(a.value) == str(b.value)


def test_the_library_exports_the_entry_point():
    assert "pgx_label_components" in _lib.ABI_SYMBOLS
    assert len(_lib.ABI_SYMBOLS) == len(set(_lib.ABI_SYMBOLS))
    header = open(HEADER).read()
    assert ("int pgx_label_components(pgx_ctx *ctx, const int32_t *labels, int64_t n, int32_t first_ignored, int32_t *comp_out,\n"
            "                         int32_t *first_out, int64_t *sizes_out, int64_t *components);") in header
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pgx_label_components")
    assert hasattr(_lib.Context, "label_components")
    long_row = int(re.search(r"#define PGX_COMPONENTS_LONG_ROW (\d+)", header).group(1))
    assert long_row == _lib.COMPONENTS_LONG_ROW == CM.LONG_ROW
    assert long_row & (long_row - 1) == 0


# ---- regroup ----------------------------------------------------------------------------------------------------------------------------
def components_of(labels, comp):
    """(first, sizes) of a hand-made comp array"""
    c = int(comp.max()) + 1
    first = np.array([np.flatnonzero(comp == j)[0] for j in range(c)], dtype=np.int32)
    sizes = np.array([(comp == j).sum() for j in range(c)], dtype=np.int64)
    assert (np.diff(first) > 0).all() if c > 1 else True        # numbered by their smallest member, as the library does
    return first, sizes


def both_regroups(labels, model_number, comp, mpn, keep):
    labels, comp = np.asarray(labels, dtype=np.int32), np.asarray(comp, dtype=np.int32)
    first, sizes = components_of(labels, comp)
    got = _components.regroup(labels, model_number, comp, first, sizes, mpn, keep)
    ref = CM.regroup(labels, model_number, comp, first, sizes, mpn, keep)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    return got


def test_regroup_hand_made_cases():
    #           0  1  2  3  4  5  6  7  8  9 10 11
    labels = [0, 0, 1, 1, 0, 0, 2, 1, 1, 0, 3, 0]
    comp = [0, 0, 1, 1, 2, 2, -1, 3, 3, 4, -1, 4]                # model 0: three components of 2 (a tie in size); model 1: two of 2
    new, parent = both_regroups(labels, 2, comp, 1, "all")
    assert parent.tolist() == [0, 0, 0, 1, 1]                    # ties in size: ascending first
    assert new.tolist() == [0, 0, 3, 3, 1, 1, 5, 4, 4, 2, 5, 2]
    new, parent = both_regroups(labels, 2, comp, 1, "largest")   # the tie goes to the smaller first
    assert parent.tolist() == [0, 1] and new.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2]
    # sizes differ: the larger first whatever its position; model 1 loses every component to the size test and is absent
    labels = [0, 1, 0, 0, 0, 1, 2, 2, 2, 9]
    comp = [0, 1, 2, 2, 2, 3, 4, 4, 4, -1]
    new, parent = both_regroups(labels, 3, comp, 2, "all")
    assert parent.tolist() == [0, 2] and new.tolist() == [2, 2, 0, 0, 0, 2, 1, 1, 1, 2]
    new, parent = both_regroups(labels, 3, comp, 1, "all")
    assert parent.tolist() == [0, 0, 1, 1, 2] and new.tolist() == [1, 2, 0, 0, 0, 3, 4, 4, 4, 5]
    new, parent = both_regroups(labels, 3, comp, 4, "largest")   # the largest fails the size test: nothing of the model is kept
    assert parent.tolist() == [] and (new == 0).all()
    # model_number = 0 and all points outliers: no components at all
    for labels in ([0, 1, 2, 3], [-1, -1, -1, -1], [5, 5, 5, 5]):
        none = np.full(4, -1, dtype=np.int32)
        got = _components.regroup(np.array(labels, dtype=np.int32), 0, none, np.zeros(0, np.int32), np.zeros(0, np.int64), 1, "all")
        ref = CM.regroup(np.array(labels), 0, none, [], [], 1, "all")
        assert got[0].tolist() == ref[0].tolist() == [0, 0, 0, 0] and len(got[1]) == len(ref[1]) == 0
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    with pytest.raises(ValueError, match="keep should be"):
        _components.regroup(np.zeros(4, np.int32), 1, none, np.zeros(0, np.int32), np.zeros(0, np.int64), 1, "biggest")


def test_regroup_random_cases():
    rng = np.random.default_rng(2024)
    kept = 0
    for case in range(200):
        n = int(rng.integers(1, 120))
        models = int(rng.integers(0, 5))
        graph = CM.random_graph(n, float(rng.choice([0.5, 1.0, 2.0])), rng, weighted=False)
        labels = rng.integers(-1, models + 2, n).astype(np.int32)
        comp, first, sizes = CM.label_components(graph[0], graph[1], labels, models)
        for keep in ("all", "largest"):
            mpn = int(rng.integers(1, 6))
            got = _components.regroup(labels, models, comp, first, sizes, mpn, keep)
            ref = CM.regroup(labels, models, comp, first, sizes, mpn, keep)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (case, keep)
            kept += len(ref[1])
    assert kept > 400                                           # the cases are not all empty


# ---- the find / link statements on std::atomic ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("components") / "libcomponents_driver.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "components_driver.cpp")])
    lib = C.CDLL(so)
    lib.cc_emu_run.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def arcs_of(graph):
    off, idx = graph[0], graph[1]
    return np.repeat(np.arange(len(off) - 1, dtype=np.int32), np.diff(off)), np.ascontiguousarray(idx, dtype=np.int32)


def run_emu(emu, n, a, b, labels, first_ignored, threads=1):
    """(comp, first, sizes) from the roots the driver returns: the root IS the smallest member, so the roots in ascending order number
    the components"""
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    root = np.full(max(n, 1), -7, dtype=np.int32)
    r = emu.cc_emu_run(n, len(a), a.ctypes.data, b.ctypes.data, labels.ctypes.data, int(first_ignored), threads, root.ctypes.data)
    assert r == 0                                               # arcs in range and parent[x] <= x everywhere
    root = root[:n]
    first, inverse, sizes = np.unique(root[root >= 0], return_inverse=True, return_counts=True)
    comp = np.full(n, -1, dtype=np.int32)
    comp[root >= 0] = inverse
    return comp, first.astype(np.int32), sizes.astype(np.int64)


def same(got, ref):
    return all(np.array_equal(g, r) for g, r in zip(got, ref)) and len(got[1]) == len(ref[1])


def test_the_statements_in_many_arc_orders_equal_the_model(emu):
    rng = np.random.default_rng(11)
    cases = 0
    for name, graph, labels, first_ignored, _ in CM.small_cases():
        ref = CM.reference(name, graph, labels, first_ignored)
        n = len(labels)
        a, b = arcs_of(graph)
        assert same(run_emu(emu, n, a, b, labels, first_ignored), ref), name
        assert same(run_emu(emu, n, a[::-1], b[::-1], labels, first_ignored), ref), name
        assert same(run_emu(emu, n, b, a, labels, first_ignored), ref), name        # every arc from its other end
        for _ in range(50):
            p = rng.permutation(len(a))
            assert same(run_emu(emu, n, a[p], b[p], labels, first_ignored), ref), name
        cases += 1
    assert cases == 24 + 16 + 6 + 2 + 60 + 2


def test_the_model_on_cases_known_by_hand():
    g = CM.grid_graph(32, 32)
    y, x = np.divmod(np.arange(1024), 32)
    comp, first, sizes = CM.label_components(g[0], g[1], (x + y) % 2, 2)
    assert np.array_equal(comp, np.arange(1024)) and np.array_equal(first, np.arange(1024)) and (sizes == 1).all()
    comp, first, sizes = CM.label_components(g[0], g[1], (x // 4) % 2, 2)
    assert first.tolist() == [0, 4, 8, 12, 16, 20, 24, 28] and (sizes == 128).all() and np.array_equal(comp, x // 4)
    comp, first, sizes = CM.label_components(g[0], g[1], np.zeros(1024), 0)
    assert (comp == -1).all() and len(first) == len(sizes) == 0
    comp, first, sizes = CM.label_components(*CM.path_graph(np.array([3, 0, 2, 1]))[:2], [0, 0, 1, 0], 2)
    assert comp.tolist() == [0, 1, 2, 0] and first.tolist() == [0, 1, 2] and sizes.tolist() == [2, 1, 1]
    comp, first, sizes = CM.label_components([0, 1, 1, 2], [2, 2], [0, 0, 0], 1)    # an asymmetric row joins, a self arc does not matter
    assert comp.tolist() == [0, 1, 0] and sizes.tolist() == [2, 1]


@pytest.mark.parametrize("kind", ["chain", "chain-permuted", "star-first", "star-last", "random-2", "random-8"])
def test_eight_threads_on_a_shuffled_arc_list_equal_the_model(emu, kind):
    n = 10000
    rng = np.random.default_rng(len(kind))
    if kind.startswith("chain"):
        graph = CM.path_graph(np.arange(n) if kind == "chain" else rng.permutation(n))
        labels, first_ignored = np.zeros(n, dtype=np.int32), 1
    elif kind.startswith("star"):
        hub = 0 if kind == "star-first" else n - 1
        graph = CM.hub_graph(n, [hub], [[v for v in range(n) if v != hub]])
        labels, first_ignored = np.zeros(n, dtype=np.int32), 1
    else:
        graph = CM.random_graph(n, int(kind.split("-")[1]), rng, weighted=False)
        labels, first_ignored = rng.integers(0, 3, n).astype(np.int32), 3 if kind == "random-2" else 2
    ref = CM.label_components(graph[0], graph[1], labels, first_ignored)
    a, b = arcs_of(graph)
    for _ in range(5):
        p = rng.permutation(len(a))
        assert same(run_emu(emu, n, a[p], b[p], labels, first_ignored, threads=8), ref)
