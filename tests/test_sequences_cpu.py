"""The model of the C ABI (tests/ctx_model.py) and the committed call sequences (tests/soak_sequences.py), checked without a GPU:
the generator covers the contract, every rule of the model is contradicted by some committed sequence once it is switched off, and the
judge finds nothing between the true model and itself.  The op streams are exactly those tests/test_gpu_sequences.py runs on the
device, so the evidence that a rule is under test comes from here - no modified library ever runs."""
import functools

import numpy as np
import pytest

import ctx_model as CM
import soak_sequences as S

WHICH = S.SEEDS + tuple(S.HISTORIES)


@functools.lru_cache(maxsize=None)
def _sequence(which):
    ops = S.sequence(which)
    return ops, S.model_outcomes(ops)


def test_a_sequence_is_a_pure_function_of_its_seed():
    a, b = S.generate(S.SEEDS[0]), S.generate(S.SEEDS[0])
    assert len(a) == len(b) >= S.OPS_PER_SEQUENCE and all(x[0] == y[0] and S.same(x[1], y[1]) for x, y in zip(a, b))
    assert all(set(op[1]) <= {k for k in CM.ContextModel.__dict__["op_" + op[0]].__code__.co_varnames} for op in a)   # plain data: name + arguments


def test_the_generator_covers_the_contract():
    per_op, per_refusal, ns, share, identical = S.coverage(S.SEEDS)
    assert set(per_op) == set(S.OP_NAMES)
    assert not {k: v for k, v in per_op.items() if v < 3}, "every op name occurs at least three times"
    assert not [k for k, v in per_refusal.items() if v < 1], "every refusal class occurs"
    assert ns == set(S.N_LIST), "every n of the size list has been resident"
    assert max(share.values()) <= 0.25, f"at most one call in four is refused: {share}"
    assert identical >= 1, "an expansion answered after an identical one with no writer, table or graph in between"
    for which in S.HISTORIES:                                    # the written-out histories keep to the same share
        outs = _sequence(which)[1]
        assert sum(o[0] == "refused" for o in outs) * 4 <= len(outs)


def test_no_refusal_outside_the_documented_ones_is_drawn():
    for which in WHICH:
        for op, out in zip(*_sequence(which)):
            assert out[0] == "ok" or out[1] in CM.REFUSALS, (which, op[0], out[1])


@pytest.mark.parametrize("which", WHICH)
def test_the_judge_finds_nothing_between_the_model_and_itself(which):
    ops, outs = _sequence(which)
    assert S.judge(CM.ContextModel(), ops, outs) == []


@pytest.mark.parametrize("rule", sorted(CM.RULES))
def test_every_rule_is_exercised(rule):
    """a rule that no committed sequence can tell from its absence is not being tested: the fix is the generator or the seeds"""
    found = [(which,) + S.judge(CM.ContextModel(off={rule}), *_sequence(which))[0] for which in WHICH
             if S.judge(CM.ContextModel(off={rule}), *_sequence(which))]
    assert found, f"no committed sequence contradicts the model without '{rule}' ({CM.RULES[rule]})"


def test_the_judge_sees_what_it_is_for():
    """the comparisons themselves: a flipped mask bit, a sum off by 2e-9, a refusal of another class, an accepted refused call"""
    ops, outs = _sequence(S.SEEDS[0])
    i = next(k for k, (op, o) in enumerate(zip(ops, outs)) if o[0] == "ok" and isinstance(o[1], dict) and "f_values" in o[1] and np.any(o[1]["f_values"] != 0))
    r = next(k for k, o in enumerate(outs) if o[0] == "refused")
    for change in ("counts", "f_values", "class", "accepted", "short"):
        bent = list(outs)
        if change == "counts":
            res = dict(bent[i][1], counts=bent[i][1]["counts"] + 1)
            bent[i] = ("ok", res)
        elif change == "f_values":
            bent[i] = ("ok", dict(bent[i][1], f_values=bent[i][1]["f_values"] * (1.0 + 2e-9)))
        elif change == "class":
            bent[r] = ("refused", "pgx_nothing: some other sentence")
        elif change == "accepted":
            bent[r] = ("ok", None)
        else:
            bent = bent[:-3]
        found = S.judge(CM.ContextModel(), ops, bent)
        assert len(found) == 1 and found[0][0] == {"counts": i, "f_values": i, "class": r, "accepted": r, "short": len(ops) - 3}[change], (change, found)
    close = list(outs)
    close[i] = ("ok", dict(close[i][1], f_values=close[i][1]["f_values"] * (1.0 + 2e-10)))     # inside the project's bound: REL = 1e-9
    scale_ok = S.judge(CM.ContextModel(), ops, close)
    assert scale_ok == [] or all(f[0] != i or "f_values" not in f[2] for f in scale_ok)
