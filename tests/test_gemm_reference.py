"""The acceptance check of the GEMM family (tests/gemm_reference.py) can fail: on exactly the cases tests/test_gpu_gemm_abi.py
runs, the float32 CPU evaluation passes it and every listed mistake is refused.  Also holds the K_OP table to its rule
(constant = 4 x the float32 evaluation's measured error, rounded up), shows that the five stride layouts of every shape really
differ, and runs the float32 stand-in through the strided ap_layernorm / ap_stream_init / ap_rowstats_finalize cases."""
import math

import pytest
import torch

from tests import gemm_reference as G
from tests import vit_ops_reference as R

EXPECTED = {  # epilogue -> the mutations that must have been refused at least once
    epi: {"a_stride_k", "w_stride_k", "out_stride_n", "last_ktile_dropped", "first_ktile_twice", "bias_next_tile"} | extra
    for epi, extra in (("bias", set()), ("gelu", set()), ("quick_gelu", set()), ("gelu_tanh", set()), ("resid", {"resid_overwrites"}),
                       ("resid_gamma", {"resid_overwrites", "gamma_ignored"}), ("norm", {"stats_swapped"}), ("norm_gelu", {"stats_swapped"}),
                       ("norm_quick_gelu", {"stats_swapped"}), ("norm_gelu_tanh", {"stats_swapped"}),
                       ("norm_swiglu", {"stats_swapped", "swiglu_halves_swapped"}),
                       ("resid_stats", {"partial_neighbour_group", "partial_unrounded_row"}))}


MUTATED_ROWS = 1024


def _hold_to_rule(key, value):
    recorded, constant = G.K_OP[key]
    print(f"k_op {key}: measured {value:.3f}, recorded {recorded}, constant {constant}")
    assert constant == math.ceil(4 * recorded), "the constant is 4 x the recorded measurement, rounded up"
    # torch's float32 summation order depends on the host's vector width: a band, not an equality -- and two-sided, so that a
    # constant cannot stay loose after the inputs changed
    assert 0.67 * recorded <= value <= 1.5 * recorded, f"{key}: the float32 evaluation measures {value:.3f}: record it"


@pytest.mark.parametrize("epi", sorted(G.EPI))
def test_float32_evaluation_passes_and_every_mutation_is_rejected(epi):
    seen, measured, measured_partial, count = set(), 0.0, 0.0, 0
    for dt in [d for d, e in G.GROUPS if e == epi]:
        differ = total = 0
        for case in G.cases(dt, epi):
            a, count = case.args, count + 1
            o = G.ref_gemm(a)["out"]
            o32 = G.ref_gemm(a, torch.float32)["out"]
            k = G.k_of(a)
            stand_in, stored64 = G.as_output(o32, a), G.as_output(o, a)
            measured = max(measured, G.measure_k(o32, o))
            bad = G.failures(stand_in, o, k)
            assert bad == 0, f"{case.id}: the float32 evaluation fails the check ({bad} elements)"
            if epi == "resid_stats":
                d = int((G.bits(stand_in) != G.bits(stored64)).sum())
                differ, total = differ + d, total + stand_in.numel()
                assert G.share_ok(d, stand_in.numel(), pooled=False), f"{case.id}: {d} of {stand_in.numel()} differ from T(x0 + T(d64))"
                kp = G.k_of(a, "partial")
                wantp = G.ref_partial(a, stand_in)
                p32 = G.ref_partial(a, stand_in, torch.float32)
                measured_partial = max(measured_partial, G.measure_k(p32, wantp))
                assert G.failures(p32.value.float(), wantp, kp) == 0, f"{case.id}: the float32 partial sums fail the check"
            if a["M"] > MUTATED_ROWS:             # the seam case: its mutations on the first rows alone (gemm_reference.head)
                a = G.head(a, MUTATED_ROWS)
                o = G.ref_gemm(a)["out"]
                stored64 = G.as_output(o, a)
            for m in case.mutations:
                if m == "out_stride_n":
                    bad = G.failures(G.stored_at(stored64, a, a["cols"]), o, k)
                elif m.startswith("partial_"):
                    wrong = G.ref_partial(a, stored64, torch.float64, m, unrounded=o.value)
                    bad = G.failures(wrong.value.float(), G.ref_partial(a, stored64), G.k_of(a, "partial"))
                else:
                    bad = G.failures(G.as_output(G.ref_gemm(a, torch.float64, m)["out"], a), o, k)
                assert bad > 0, f"{case.id}: mutation {m} passes the check -- the inputs are too weak"
                seen.add(m)
            a.pop("_cache", None)
            case.args.pop("_cache", None)
        assert epi != "resid_stats" or G.share_ok(differ, total, pooled=True), (dt, differ, total)
    assert count > 0 and seen == EXPECTED[epi], (epi, EXPECTED[epi] ^ seen)
    _hold_to_rule(epi, measured)
    if epi == "resid_stats":
        _hold_to_rule("resid_stats_partial", measured_partial)


def test_every_listed_mutation_belongs_to_some_epilogue():
    assert set().union(*EXPECTED.values()) == set(G.MUTATIONS)
    assert set(EXPECTED) == set(G.EPI) and set(G.K_OP) == set(G.EPI) | {"resid_stats_partial"}


@pytest.mark.parametrize("dt", G.ALL, ids=str)
def test_the_stride_layouts_really_differ_and_the_shapes_cover_the_kernels(dt):
    """Per shape: dense, each stride padded alone, all three padded by different amounts that are no powers of two; the padding
    holds the NaN pattern and 256 NaN rows follow A; the shape sets contain what the kernels' paths need."""
    by_shape = {}
    for epi in ("bias", "resid", "norm_swiglu"):
        if (dt, epi) not in G.GROUPS:
            continue
        for case in G.cases(dt, epi):
            a = case.args
            M, N, K = a["M"], a["N"], a["K"]
            by_shape.setdefault((epi, M, N, K), set()).add((a["lda"] > K, a["ldw"] > K, a["ldo"] > a["cols"]))
            es = a["A"].element_size()
            assert a["lda"] * es % 16 == 0 and a["ldw"] * es % 16 == 0 and a["ldo"] % 4 == 0
            assert tuple(a["A"].shape) == (M + 256, a["lda"]) and G.padding_is_untouched(a["A"], M, K)
            assert tuple(a["W"].shape) == (N, a["ldw"]) and G.padding_is_untouched(a["W"], N, K)
            assert not bool(a["A"][:M, :K].isnan().any()) and not bool(a["W"][:N, :K].isnan().any())
            if a["layout"] == "all":
                pads = {a["lda"] - K, a["ldw"] - K, a["ldo"] - a["cols"]}
                assert len(pads) == 3 and all(p & (p - 1) for p in pads)
    full = {(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True)}
    seam = (G.seam_rows(256), 768, 128)
    for (epi, *shape), combos in by_shape.items():
        assert combos == (full if tuple(shape) != seam else {(True, True, True)}), (epi, shape, combos)
    kt = G.ktile(dt)
    s128 = G.shapes128(dt)
    assert {m for m, _, _ in s128} == {1, 64, 65, 128, 129, 257} and {n for _, n, _ in s128} == {128, 384, 640}
    assert {k for _, _, k in s128} == {kt, 2 * kt, 3 * kt, 5 * kt} and s128[0] == (1, 128, kt) and (257, 640, kt) in s128
    assert {m for m, _, _ in G.SHAPES256} == {1, 255, 256, 257, 513} and {n for _, n, _ in G.SHAPES256} == {256, 768, 3072}
    assert {k for _, _, k in G.SHAPES256} == {128, 256, 384}
    for cus in (256, 304, 64):
        assert -(-G.seam_rows(cus) // 256) * 3 > cus and G.seam_rows(cus) % 256 == 5


def test_takes256_follows_the_layout_rule():
    for dt, epi in ((torch.float16, "bias"), (torch.bfloat16, "resid"), (torch.float32, "bias")):
        for case in G.cases(dt, epi):
            a = case.args
            want = dt != torch.float32 and a["N"] % 256 == 0 and a["K"] % 128 == 0
            assert G.takes256(a) == want, case.id           # every layout of the persistent kernel's shapes is one it admits


def test_strided_layernorm_and_stream_cases_pass_in_float32():
    """The float32 evaluation passes the check with the constants of tests/vit_ops_reference.py on the strided ap_layernorm
    cases, the ap_stream_init cases and the ap_rowstats_finalize cases."""
    count = 0
    for case in G.cases_layernorm_strided():
        a = case.args
        assert a["stride"] > a["dim"] and a["stride"] % 4 == 0 and bool(a["x"][:, a["dim"]:].isnan().all())
        want, got = R.ref_add2_layernorm(a), R.ref_add2_layernorm(a, torch.float32)
        o = want["out"]
        assert R.failures(got["out"].value.to(o.dtype), o, R.K_OP["add2_layernorm"][1]) == 0, case.id
        assert R.same_bits(want["x"].value, a["x"])
        count += 1
    assert count == 27
    k = R.K_OP["rowstats_finalize_cls"][1]
    for case in G.cases_stream_init():
        want, got = G.ref_stream_init(case.args), G.ref_stream_init(case.args, torch.float32)
        assert R.failures(got["rowstats"].value.float(), want["rowstats"], k) == 0, case.id
        assert R.same_bits(want["x"].value, case.args["tok"].to(case.args["dtype"]))
    for case in G.cases_rowstats_finalize():
        want, got = R.ref_rowstats_finalize_cls(case.args), R.ref_rowstats_finalize_cls(case.args, torch.float32)
        assert set(want) == {"rowstats"}
        assert R.failures(got["rowstats"].value.float(), want["rowstats"], k) == 0, case.id


def test_an_extra_allowance_is_absolute_and_nothing_more():
    ref = torch.tensor([1.0, 0.0], dtype=torch.float64)
    out = G.GOut(ref, torch.float32, torch.tensor([1.0, 0.0], dtype=torch.float64), extra=torch.full((2,), 3e-5, dtype=torch.float64))
    assert G.failures(torch.tensor([1.0 + 2.9e-5, 0.0]), out, 1.0) == 0
    assert G.failures(torch.tensor([1.0 + 3.2e-5, 0.0]), out, 1.0) == 1
    assert G.failures(torch.tensor([1.0, 1e-6]), out, 1.0) == 1          # A = 0: an exact element gets no allowance
    assert G.failures(torch.tensor([float("nan"), 0.0]), out, 1.0) == 1
