"""Random call sequences on one context against the model of the C ABI (tests/ctx_model.py, tests/soak_sequences.py).

What the sequence tests hold: over unscripted histories of every single-GPU call that touches or reads resident state, the device
accepts and refuses what include/pgx.h says (refusal by refusal, matched by its text), returns what the oracle computes from the
resident state the contract lists (integers, masks, labels, energies bit for bit, floating sums to 1e-9), and - at up to eight
points of every sequence - gives bit for bit what a fresh context that has seen only that state gives.  The same under
PGX_MF_DONE_VERIFY=1, PGX_MF_MEMO=0 and PGX_SETPOINTS_HOST=1.  What they do not hold: the communicator calls and multi-rank state.
tests/test_sequences_cpu.py shows, without a GPU, that every rule of the model is needed to pass."""
import pytest

import soak_sequences as S
from ctx_model import ContextModel

pytestmark = pytest.mark.gpu

WHICH = S.SEEDS + tuple(S.HISTORIES)
_DEFAULT = {}          # which -> the outcomes on the session's context under the default switches


def _on(ctx, ops, checkpoints=S.MAX_CHECKPOINTS):
    res = S.run(ctx, ops, checkpoints=checkpoints)
    assert res["stopped"] is None, f"op {res['stopped'][0]} ({ops[res['stopped'][0]][0]}) failed with something other than PGX_ERR_INVALID: {res['stopped'][1]}"
    return res


def _default(gpu_ctx, which, ops):
    if which not in _DEFAULT:
        _DEFAULT[which] = _on(gpu_ctx, ops, checkpoints=0)["outcomes"]
    return _DEFAULT[which]


@pytest.mark.parametrize("which", WHICH)
def test_sequences_agree_with_the_contract(gpu_ctx, oracle, which):
    """the committed sequences on the session's context, which lives across them (and across every other test) on purpose"""
    ops = S.sequence(which)
    res = _on(gpu_ctx, ops)
    _DEFAULT[which] = res["outcomes"]
    assert S.judge(ContextModel(), ops, res["outcomes"]) == []
    assert len(res["checkpoints"]) >= 1 and [i for i, ok in res["checkpoints"] if not ok] == [], "a fresh context gives other bits at these ops"


@pytest.mark.parametrize("switch", ["PGX_MF_DONE_VERIFY=1", "PGX_MF_MEMO=0"])
def test_sequences_do_not_see_the_memo_switches(gpu_ctx, oracle, monkeypatch, switch):
    """the same sequences on a context of their own with the identical-call shortcut verified by a real cycle, and with the memo and
    the shortcut off: both are invisible by contract, so every outcome - refusal texts included - is the default context's"""
    from pyprogressivex import _lib
    name, value = switch.split("=")
    monkeypatch.setenv(name, value)
    with _lib.Context(0) as ctx:
        monkeypatch.delenv(name)
        for which in WHICH:
            ops = S.sequence(which)
            got = _on(ctx, ops, checkpoints=0)["outcomes"]
            assert S.same(got, _default(gpu_ctx, which, ops)), (switch, which)
            assert S.judge(ContextModel(), ops, got) == [], (switch, which)


@pytest.mark.parametrize("seed", [S.SEEDS[0], S.SEEDS[1]])
def test_sequences_do_not_see_where_the_points_were_preprocessed(oracle, monkeypatch, seed):
    """PGX_SETPOINTS_HOST=1 (the host version of pgx_set_points' preprocessing): bitwise the outcomes of the device version, floats
    included.  On the types both versions sort (the host version builds no sorted copies for the others, which then score on
    another path: an A/B switch, not a contract)."""
    from pyprogressivex import _lib
    ops = S.generate(seed, types=S.HOST_TYPES)
    with _lib.Context(0) as device:
        want = _on(device, ops, checkpoints=0)["outcomes"]
    monkeypatch.setenv("PGX_SETPOINTS_HOST", "1")
    with _lib.Context(0) as host:
        monkeypatch.delenv("PGX_SETPOINTS_HOST")
        got = _on(host, ops, checkpoints=0)["outcomes"]
    assert S.same(got, want)
    assert S.judge(ContextModel(), ops, got) == []
