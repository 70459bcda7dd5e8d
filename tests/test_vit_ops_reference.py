"""The acceptance check of the engine building blocks (tests/vit_ops_reference.py) can fail: on the inputs and shapes
tests/test_gpu_vit_ops.py uses, the float32 CPU evaluation of every operator passes it and every listed mistake is refused.
Also holds the k_op table to its rule: constant = 4 x the float32 evaluation's measured error, rounded up."""
import math

import numpy as np
import pytest
import torch

from tests import vit_ops_reference as R

MUTATIONS = {"attention": R.FULL_MUTATIONS, "attention_cls": R.ATTN_MUTATIONS, "attn_pool": R.ATTN_MUTATIONS, "rope": R.ROPE_MUTATIONS, "swiglu": R.SWIGLU_MUTATIONS,
             "add2_layernorm": R.LN_MUTATIONS, "fold_ln": R.FOLD_LN_MUTATIONS, "fold_ls": (), "cls_stream": R.CLS_MUTATIONS,
             "cls_exact_update": R.CLS_MUTATIONS, "rowstats_finalize_cls": R.FIN_MUTATIONS}


def _as_output(outs):
    """What a kernel that computed `outs` would leave in memory: every value rounded once to its output type."""
    return {name: o.value.to(o.dtype) for name, o in outs.items()}


@pytest.mark.parametrize("op", sorted(R.REFS))
def test_float32_evaluation_passes_and_every_mutation_is_rejected(op):
    ref = R.REFS[op]
    seen, measured, measured_hot, count = set(), 0.0, 0.0, 0
    for case in R.cases(op):
        count += 1
        want = ref(case.args, torch.float64)
        got32 = ref(case.args, torch.float32)
        for name, o in want.items():
            measured = max(measured, R.measure_k(got32[name], o))
            measured_hot = max(measured_hot, R.measure_k(got32[name], o, hot=True))
            bad = R.failures(got32[name].value.to(o.dtype), o, R.k_of(op, o))
            assert bad == 0, f"{op} {case.id}: the float32 evaluation fails the check on `{name}` ({bad} elements)"
        for m in case.mutations:
            got = _as_output(ref(case.args, torch.float64, m))
            bad = sum(R.failures(got[name], o, R.k_of(op, o)) for name, o in want.items())
            assert bad > 0, f"{op} {case.id}: mutation {m} passes the check -- the inputs are too weak"
            seen.add(m)
    assert count > 0 and seen == set(MUTATIONS[op]), (op, set(MUTATIONS[op]) - seen)
    for key, value in ((op, measured), (op + "_hot", measured_hot)):
        if key in R.K_OP:
            recorded, constant = R.K_OP[key]
            print(f"k_op {key}: measured {value:.3f}, recorded {recorded}, constant {constant}")
            assert constant == math.ceil(4 * recorded), "the constant is 4 x the recorded measurement, rounded up"
            # torch's float32 summation order depends on the host's vector width: a band, not an equality -- and two-sided, so
            # that a constant cannot stay loose after the inputs changed
            assert 0.67 * recorded <= value <= 1.5 * recorded, f"{key}: the float32 evaluation measures {value:.3f}: record it"
    assert (op + "_hot" in R.K_OP) == (measured_hot > 0)


@pytest.mark.parametrize("kernel", ["tiled", "strip"])
def test_attention_rounded_weights_model_fits_the_bound(kernel):
    """A correct 16-bit kernel fits: float32 scores, keys walked in tiles of 64, weights rounded to T, row sums of the rounded
    weights (tiled kernel) or of the unrounded ones (register-strip kernel) -- with the coefficient of u(T) B at 1.  Without
    the B term the same model is refused: the term is needed, and it is not slack.  Under the strip kernel's B every listed
    mistake is refused as well (the parametrised test above holds the tiled kernel's)."""
    worst, without, count = 0.0, 0.0, 0
    for case in R.cases("attention", dtypes=R.HALF, **({"kernel": "strip", "widths": (64,)} if kernel == "strip" else {})):
        count += 1
        o = R.ref_attention(case.args)["out"]
        got = R.model_attention(case.args)
        k = R.k_of("attention", o)
        bad = R.failures(got, o, k)
        err = (got.double() - o.value).abs()
        worst = max(worst, float((err / R.tolerance(o, k)).max()))
        without = max(without, float((err / (R.tolerance(o, k) - o.weight_rounding)).max()))
        assert bad == 0, f"{case.id}: the rounded-weights model fails the check ({bad} elements)"
        if kernel == "strip":
            for m in case.mutations:
                wrong = R.ref_attention(case.args, torch.float64, m)["out"].value.to(o.dtype)
                assert R.failures(wrong, o, k) > 0, f"{case.id}: mutation {m} passes under the strip kernel's bound"
    print(f"attention, {kernel} model: {count} cases, worst |model - ref64| / bound = {worst:.3f}; without the B term {without:.1f}")
    assert count > 0 and worst <= 1.0 < without


def test_attention_cases_reach_every_branch():
    """The shapes name every last-tile body, ring depth, staging wrap and deal of query blocks the tiled kernel has, both
    shapes of the unit walk, and a rescale staircase at each width that defers, rescales and rescales on a partial last tile."""
    tokens = set(R.FULL_TOKENS)
    left = {T - (T - 1) // 64 * 64 for T in tokens}
    assert {1, 16, 17, 32, 33, 63, 64} <= left                             # NS = 1 / 2 / 4 at their limits
    assert {1, 2, 3, 4} <= {(T + 63) // 64 for T in tokens} and {T for T in tokens if (T + 63) // 64 % 4 == 3} >= {129, 191, 192, 385, 448}
    assert {((T + 31) // 32 + 7) // 8 for T in tokens} == {1, 2, 3, 4}
    assert [R.full_last_part_row0(T) // 32 for T in (257, 513, 785)] == [5, 12, 19]      # 5 + 4, 6 + 6 + 5, 7 + 6 + 6 + 6
    for hd in (64, 96, 128):
        ids = [c.id for c in R.cases("attention", dtypes=(torch.bfloat16,), widths=(hd,), max_tokens=160)]
        assert any("stair5.0+6.0" in i for i in ids) and any(i.endswith("stair5.0") for i in ids) and any("-n3-h3" in i for i in ids)
        if hd == 96:
            assert any("-w80" in i for i in ids) and any("-w80" not in i for i in ids)
    scales = {(c.args["hd"], round(c.args["scale"] * math.sqrt(c.args["hd"]), 3)) for c in R.cases("attention", dtypes=(torch.float16,), max_tokens=33)}
    assert {(64, 1.0), (64, 0.8), (128, 1.0), (128, 1.25)} <= scales


def test_add2_layernorm_strides_are_tied_to_nothing():
    """Per (types, dim): a stored update, an unstored one and a call without delta each run on dense and on padded stream
    rows, and each delta on dense and on padded rows of its own; fold weights carry NaN beyond `cols`."""
    for pair, dim in ((R.LN_PAIRS[0], 768), (R.LN_PAIRS[3], 384), (R.LN_PAIRS[4], 4096)):
        seen = set()
        for case in R.cases("add2_layernorm", pairs=(pair,), dims=(dim,)):
            a = case.args
            has = a["delta0"] is not None or a["delta1"] is not None
            seen.add(("x", has, a["store"], a["stride"] > dim))
            seen |= {(f"delta{i}", a["store"], a[f"dstride{i}"] > dim) for i in (0, 1) if a[f"delta{i}"] is not None}
        assert len(seen) == 8 + 4 + 4, sorted(seen)
    for op in ("fold_ln", "fold_ls"):
        for case in R.cases(op):
            a = case.args
            assert a["cols"] == a["ld"] or bool(a["w32"][:, a["cols"]:].isnan().any())


def test_a_nan_or_a_wrong_bit_never_passes():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    out = R.Out(ref, torch.float16, torch.ones(3, dtype=torch.float64))
    assert R.failures(ref.to(torch.float16), out, 4.0) == 0
    assert R.failures(torch.tensor([1.0, float("nan"), 0.0], dtype=torch.float16), out, 4.0) == 1
    assert R.failures(torch.tensor([1.0, -2.0, 1e-3], dtype=torch.float16), out, 4.0) == 1
    exact = R.Out(torch.tensor([1.0, -0.0]), torch.float32)
    assert R.failures(torch.tensor([1.0, -0.0]), exact, 0.0) == 0
    assert R.failures(torch.tensor([1.0, 0.0]), exact, 0.0) == 1          # the sign of zero is a bit too
    masked = R.Out(ref, torch.float16, torch.ones(3, dtype=torch.float64), torch.tensor([False, True, False]))
    assert R.failures(torch.tensor([1.0, -2.002, 0.0], dtype=torch.float16), masked, 4.0) == 1
    # half an ulp passes, a whole ulp does not
    one = R.Out(torch.tensor([1.0], dtype=torch.float64), torch.float16, torch.zeros(1, dtype=torch.float64))
    assert R.failures(torch.tensor([1.0 + 2.0 ** -10], dtype=torch.float16), one, 0.0) == 1
    assert R.U[torch.float16] == 2.0 ** -11 and R.U[torch.bfloat16] == 2.0 ** -8 and R.U[torch.float32] == 0.0
    assert R.FLOOR[torch.float16] == float(np.finfo(np.float16).smallest_subnormal) / 2


def test_cls_mean_pool_check_rejects_its_mutations():
    seen = set()
    for case in R.cases("cls_mean_pool"):
        row0, mean = R.ref_cls_mean_pool(case.args)
        assert R.pool_mean_ok(mean.float(), mean)
        assert not R.pool_mean_ok(torch.from_numpy(np.nextafter(np.nextafter(mean.float().numpy(), np.float32(np.inf)), np.float32(np.inf))), mean)
        for m in case.mutations:
            _, wrong = R.ref_cls_mean_pool(case.args, m)
            assert not R.pool_mean_ok(wrong.float(), mean), (case.id, m)
            seen.add(m)
    assert seen == set(R.POOL_MUTATIONS)


def test_exact_references_state_the_contract():
    """chw_to_patchrows against explicit indexing, the SwiGLU row order against its definition, stream_to_f32 exact."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 28, 28, generator=g)
    rows = R.ref_chw_to_patchrows(x, 14, torch.float16)
    assert rows.shape == (2 * 2 * 2, 3 * 14 * 14)
    for img, c, y, xx in ((0, 0, 0, 0), (1, 2, 27, 13), (1, 1, 14, 15), (0, 2, 13, 27)):
        py, ky, px, kx = y // 14, y % 14, xx // 14, xx % 14
        assert rows[(img * 2 + py) * 2 + px, (c * 14 + ky) * 14 + kx] == x[img, c, y, xx].to(torch.float16)
    h = 96
    src = [R.swiglu_source_row(r, h) for r in range(2 * h)]
    assert sorted(src) == list(range(2 * h))
    assert src[:32] == list(range(32)) and src[32:64] == list(range(h, h + 32)) and src[64:96] == list(range(32, 64))
    s = torch.randn(3, 12, generator=g).to(torch.bfloat16)
    assert torch.equal(R.ref_stream_to_f32(s, 8), s[:, :8].to(torch.float32))


def test_attention_scaled_inputs_tell_the_scales_apart():
    """An 80-wide head stored 96 wide: 1 / sqrt(96) instead of 1 / sqrt(80) moves the output by more than the tolerance, and
    the outputs stay within the magnitude the tolerance was written for."""
    for dt in R.HALF:
        qkv = R.attention_scaled_inputs(dt, 3, 65, 3, 96, 80, 0)
        right = R.ref_attention_scaled(qkv, 3, 65, 3, 96, 80, 1 / math.sqrt(80))
        wrong = R.ref_attention_scaled(qkv, 3, 65, 3, 96, 80, 1 / math.sqrt(96))
        assert right.abs().max() <= 6 and (right[:, 80:96] == 0).all()
        assert (right - wrong).abs().max() > R.ATTENTION_SCALED_TOL[dt]
        assert (right.to(dt).double() - right).abs().max() <= R.ATTENTION_SCALED_TOL[dt]
