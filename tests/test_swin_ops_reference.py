"""The acceptance check of the two Swin operators (tests/swin_ops_reference.py) can fail: on the inputs and shapes
tests/test_gpu_swin_ops.py uses, the float32 CPU evaluation passes it and every listed mistake is refused.  Also holds the
K_OP table to its rule (constant = 4 x the float32 evaluation's measured error, rounded up), the case ids to being unique, the
inputs to what their description promises, and the restated launch partition to the figures the GPU test states."""
import math

import pytest
import torch

from tests import swin_ops_reference as R


def _as_output(outs):
    """What a kernel that computed `outs` would leave in memory: every value rounded once to its output type."""
    return {name: o.value.to(o.dtype) for name, o in outs.items()}


@pytest.mark.parametrize("op", sorted(R.REFS))
def test_float32_evaluation_passes_and_every_mutation_is_rejected(op):
    ref = R.REFS[op]
    seen, ids, measured, measured_hot = set(), set(), 0.0, 0.0
    for case in R.cases(op):
        assert case.id not in ids, f"{op}: case id {case.id} twice"
        ids.add(case.id)
        want = ref(case.args, torch.float64)
        got32 = ref(case.args, torch.float32)
        for name, o in want.items():
            measured = max(measured, R.measure_k(got32[name], o))
            measured_hot = max(measured_hot, R.measure_k(got32[name], o, hot=True))
            bad = R.failures(got32[name].value.to(o.dtype), o, R.k_of(op, o))
            assert bad == 0, f"{op} {case.id}: the float32 evaluation fails the check on `{name}` ({bad} elements)"
        assert set(case.mutations) <= set(R.MUTATIONS[op])
        for m in case.mutations:
            got = _as_output(ref(case.args, torch.float64, m))
            bad = sum(R.failures(got[name], o, R.k_of(op, o)) for name, o in want.items())
            assert bad > 0, f"{op} {case.id}: mutation {m} passes the check -- the inputs are too weak"
            seen.add(m)
    assert ids and seen == set(R.MUTATIONS[op]), (op, set(R.MUTATIONS[op]) - seen)
    for key, value in ((op, measured), (op + "_hot", measured_hot)):
        if key in R.K_OP:
            recorded, constant = R.K_OP[key]
            print(f"k_op {key}: measured {value:.3f}, recorded {recorded}, constant {constant}")
            assert constant == math.ceil(4 * recorded), "the constant is 4 x the recorded measurement, rounded up"
            # torch's float32 summation order depends on the host's vector width: a band, not an equality -- and two-sided, so
            # that a constant cannot stay loose after the inputs changed
            assert 0.67 * recorded <= value <= 1.5 * recorded, f"{key}: the float32 evaluation measures {value:.3f}: record it"
    assert (op + "_hot" in R.K_OP) == (measured_hot > 0)


def test_window_attention_inputs_are_what_their_description_promises():
    """Per case: a whole hot head (scores of 95 and 94) beside ordinary heads below HOT_SCORE, flat rows, and -- shifted cases
    -- the query whose masked keys lie about 100 above the keys of its own region."""
    for case in R.cases("window_attention", dtypes=(torch.float16,)):
        a = case.args
        n, h, w, heads, shift = a["n"], a["h"], a["w"], a["heads"], a["shift"]
        out = R.ref_window_attention(a)["out"]
        hot = out.hot.view(n, h, w, heads, R.HD)
        assert bool(hot[n - 1, :, :, heads - 1].all()), case.id                 # the hot head, every token of it
        assert int(hot[..., 0].sum()) <= (h * w + (1 if shift else 0)), case.id    # ... and nothing else but the mask query
        x = a["qkv"].double().view(n, h, w, 3, heads, R.HD)
        s = torch.einsum("nyxhc,nvuhc->nhyxvu", x[:, :, :, 0], x[:, :, :, 1]) * R.HD ** -0.5
        assert 90.0 < float(s[n - 1, heads - 1].max()) < 100.0, case.id
        if shift:
            # the mask query sits at rolled position (h - 7, w - 1) of image 0, head 0: source pixel + shift
            row = s[0, 0, (h - R.WIN + shift) % h, (w - 1 + shift) % w]
            assert float(row.max()) > 95.0 and int((row > 50.0).sum()) == 2, case.id
            assert "mask_minus_inf" in case.mutations
    assert [R.run_plan(*c[:3], c[4]) for c in R.WA_GRID] == [(nwin * c[2], 1, nwin, 1, -(nwin * c[2]) % 4)
                                                            for c in R.WA_GRID for nwin in [c[4] * (c[0] // 7) * (c[1] // 7)]]


def test_run_plan_restates_the_launcher():
    """(items, wpw, runs, last run, idle waves) of the shapes the run tests use, and of the encoder's stages at batch 256."""
    assert R.run_plan(7, 7, 3, 2731) == (8193, 2, 1366, 1, 2)
    assert R.run_plan(14, 7, 1, 4097) == (8194, 2, 4097, 2, 3)
    assert R.run_plan(14, 14, 3, 1025) == (12300, 3, 1367, 2, 3)
    assert [R.run_plan(s, s, heads, 256)[1] for s, heads in ((56, 3), (28, 6), (14, 12), (7, 24))] == [8, 6, 3, 1]
    assert R.run_plan(56, 56, 3, 16)[1] == 1 and R.run_plan(14, 14, 12, 16)[1] == 1


def test_the_p_rounding_term_is_counted_and_only_for_16_bit_outputs():
    case = next(iter(R.cases("window_attention", dtypes=(torch.float32,))))
    o = R.ref_window_attention(case.args)["out"]
    plain = R.k_of("window_attention", o)
    assert set(plain.unique().tolist()) == {R.K_OP["window_attention"][1], R.K_OP["window_attention_hot"][1]}
    o16 = R.SoftmaxOut(o.value, torch.float16, o.A, hot=o.hot, pabs=o.pabs)
    extra = (R.k_of("window_attention", o16) - plain) * 2.0 ** -24 * o.A
    assert torch.allclose(extra, 2.0 ** -11 * o.pabs, rtol=1e-12, atol=0.0)
    assert bool((o.pabs <= o.A * (1 + 1e-12)).all()) and bool((o.pabs >= o.value.abs() * (1 - 1e-12)).all())
