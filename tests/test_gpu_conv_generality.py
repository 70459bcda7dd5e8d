"""The convolution family (conv.hip, convnext.hip) at the generality the header promises, not only at the layer tuples of the
shipped networks: non-square inputs, every kernel size / stride / padding the launcher admits, channel counts whose 16-byte
chunks straddle taps inside one K step, every M tail, the multi-segment path and the whole lanes-per-pixel ladder of the fused
depthwise kernel.  References are float64 on the CPU from the operands as rounded to T; errors are judged element by element
(convolutions, pools) or pixel by pixel (LayerNorm outputs), never by one norm over the tensor.

Convolution bound, element-wise (derived): K products and additions in f32, then one rounding to T
    |got - ref| <= (K + 4) * 2^-24 * (conv(|x|, |w|, |b|) + |resid|) + u_T * |ref| * 1.001      (+ 3e-5 under the erf GELU)
with u_T = 2^-24 / 2^-11 / 2^-8."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import DT, _conv_bound_ratio, _lib
from tests.test_gpu_convnext import EPS, OP_TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
DTYPES = ["float32", "float16", "bfloat16"]
SENT = 7.0
GUARD = 64


def _bytes_equal(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _guarded(dt, count):
    return torch.full((count + GUARD,), SENT, dtype=dt, device=DEV)


def _guard_ok(buf, count):
    return bool((buf[count:].float() == SENT).all())


# (ex, ksize, stride, pad, cin, cout, h, w, n, act, resid): ex = ap_conv2d_nhwc_ex (act 0 none / 1 ReLU / 2 GELU), else
# ap_conv2d_nhwc (act = its relu flag).  M = n * Ho * Wo is noted where it is one of the tile edges.
CONV_CASES = [
    (0, 1, 1, 0, 8, 64, 1, 1, 1, 0, 0),          # M = 1
    (0, 1, 1, 0, 24, 64, 1, 31, 1, 1, 1),        # M = 31
    (0, 1, 1, 0, 40, 192, 1, 127, 1, 0, 1),      # M = 127
    (0, 1, 2, 0, 72, 64, 16, 31, 1, 1, 0),       # M = 8 * 16 = 128
    (0, 1, 3, 0, 136, 64, 7, 127, 1, 0, 0),      # M = 3 * 43 = 129
    (0, 2, 1, 0, 24, 64, 5, 9, 2, 1, 1),
    (0, 2, 2, 1, 40, 192, 7, 5, 3, 0, 0),
    (0, 2, 1, 1, 8, 64, 1, 3, 1, 0, 0),          # h < ksize
    (0, 3, 1, 0, 24, 64, 5, 33, 1, 1, 0),
    (0, 3, 1, 2, 72, 64, 2, 9, 1, 0, 1),         # pad = ksize - 1, h < ksize
    (0, 3, 2, 1, 136, 192, 9, 14, 2, 1, 1),
    (0, 3, 3, 1, 40, 64, 11, 6, 1, 0, 0),
    (0, 3, 4, 2, 24, 64, 13, 21, 1, 1, 0),
    (0, 4, 1, 0, 8, 64, 4, 35, 1, 0, 0),
    (0, 4, 4, 0, 24, 192, 12, 20, 5, 0, 1),
    (0, 4, 2, 3, 40, 64, 3, 8, 1, 1, 0),         # pad = ksize - 1, h < ksize
    (0, 4, 3, 1, 72, 64, 10, 7, 2, 0, 0),
    (0, 5, 1, 0, 24, 64, 5, 35, 1, 0, 0),        # M = 31
    (0, 5, 1, 4, 8, 64, 2, 6, 1, 1, 1),          # pad = ksize - 1
    (0, 5, 2, 1, 40, 64, 9, 12, 3, 0, 1),
    (0, 5, 3, 2, 136, 64, 8, 17, 1, 1, 0),
    (0, 7, 1, 0, 8, 64, 7, 9, 1, 0, 0),
    (0, 7, 2, 3, 24, 64, 30, 45, 1, 1, 0),       # M = 345
    (0, 7, 4, 6, 40, 64, 3, 5, 2, 0, 0),         # pad = ksize - 1
    (0, 7, 3, 1, 72, 192, 6, 11, 1, 0, 1),       # h < ksize
    (0, 3, 1, 1, 64, 64, 40, 70, 1, 1, 1),       # M = 2800
    (1, 1, 1, 0, 24, 32, 1, 127, 1, 2, 0),       # M = 127
    (1, 1, 1, 0, 136, 96, 8, 16, 1, 2, 1),       # M = 128
    (1, 2, 2, 0, 40, 160, 6, 86, 1, 0, 0),       # M = 129
    (1, 2, 2, 1, 72, 32, 5, 3, 2, 1, 1),
    (1, 3, 1, 2, 8, 96, 1, 1, 1, 2, 0),          # a 1 x 1 image under a 3 x 3 kernel, pad 2
    (1, 3, 2, 0, 24, 160, 7, 9, 2, 0, 1),
    (1, 4, 4, 0, 8, 96, 16, 28, 1, 0, 0),
    (1, 4, 3, 3, 40, 32, 2, 9, 1, 2, 1),
    (1, 5, 4, 1, 72, 96, 7, 23, 1, 1, 0),
    (1, 5, 1, 4, 24, 160, 3, 4, 1, 0, 1),
    (1, 7, 1, 1, 136, 32, 5, 8, 1, 2, 0),
    (1, 7, 2, 6, 8, 96, 9, 4, 1, 0, 0),
    (1, 3, 3, 1, 40, 160, 31, 1, 1, 1, 0),       # w = 1
    (1, 1, 4, 0, 72, 96, 31, 1, 1, 1, 1),
    (1, 1, 1, 0, 8, 32, 31, 1, 1, 0, 0),         # M = 31
    (1, 2, 1, 0, 24, 96, 2, 2, 1, 2, 1),         # M = 1
]


def _out_hw(case):
    _, k, s, p, _, _, h, w, _, _, _ = case
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def test_conv_cases_cover_what_the_header_admits():
    col = lambda i: {c[i] for c in CONV_CASES}
    assert col(1) == {1, 2, 3, 4, 5, 7} and col(2) == {1, 2, 3, 4}
    assert col(4) >= {8, 24, 40, 72, 136}
    assert {c[5] for c in CONV_CASES if not c[0]} >= {64, 192} and {c[5] for c in CONV_CASES if c[0]} >= {32, 96, 160}
    assert {c[3] for c in CONV_CASES} >= {0, 1} and any(c[3] == c[1] - 1 and c[1] > 2 for c in CONV_CASES)
    assert any(c[6] < c[1] or c[7] < c[1] for c in CONV_CASES) and sum(c[6] != c[7] for c in CONV_CASES) >= 36
    ms = {c[8] * _out_hw(c)[0] * _out_hw(c)[1] for c in CONV_CASES}
    assert ms >= {1, 31, 127, 128, 129} and max(ms) > 2000
    for ex in (0, 1):
        assert {(c[9], c[10]) for c in CONV_CASES if c[0] == ex} >= {(a, r) for a in ((0, 1, 2) if ex else (0, 1)) for r in (0, 1)}


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "ex%d_k%d_s%d_p%d_cin%d_cout%d_%dx%d_n%d_act%d_r%d" % c)
def test_conv2d_general_geometry(case, dtype_name):
    ex, k, stride, pad, cin, cout, h, w, n, act, with_resid = case
    lib, L = _lib()
    dt, code = DT[dtype_name]
    g = torch.Generator().manual_seed(k * 1000 + cin + cout + 7 * h + w)
    x = torch.randn(n, cin, h, w, generator=g).to(dt)
    wt = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).to(dt)
    b = 0.1 * torch.randn(cout, generator=g)
    ho, wo = _out_hw(case)
    r = torch.randn(n, cout, ho, wo, generator=g).to(dt) if with_resid else None
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = wt.permute(0, 2, 3, 1).contiguous().to(DEV)
    rd = r.permute(0, 2, 3, 1).contiguous().to(DEV) if r is not None else None
    bd = b.to(DEV)
    count = n * ho * wo * cout
    fn = L.ap_conv2d_nhwc_ex if ex else L.ap_conv2d_nhwc
    bufs = []
    for _ in range(2):                                   # an LDS pipeline: two launches, the same bits
        buf = _guarded(dt, count)
        lib.check(fn(code, xd.data_ptr(), n, h, w, cin, wd.data_ptr(), bd.data_ptr(), cout, k, stride, pad,
                     rd.data_ptr() if rd is not None else None, act, buf.data_ptr(), lib.current_stream_ptr(DEV)), "conv2d")
        torch.cuda.synchronize()
        bufs.append(buf)
    assert _bytes_equal(bufs[0], bufs[1])
    assert _guard_ok(bufs[0], count)
    got = bufs[0][:count].view(n, ho, wo, cout).float().cpu().permute(0, 3, 1, 2)
    ratio = _conv_bound_ratio(got, x, wt, b, stride, pad, r, act, dtype_name)
    print(f"CONV {case} {dtype_name}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_conv2d_with_no_images_writes_nothing(dtype_name):
    lib, L = _lib()
    dt, code = DT[dtype_name]
    x = torch.zeros(8 * 8 * 8, dtype=dt, device=DEV)
    wt = torch.zeros(64 * 9 * 8, dtype=dt, device=DEV)
    b = torch.zeros(64, device=DEV)
    for fn in (L.ap_conv2d_nhwc, L.ap_conv2d_nhwc_ex):
        buf = _guarded(dt, 0)
        assert fn(code, x.data_ptr(), 0, 8, 8, 8, wt.data_ptr(), b.data_ptr(), 64, 3, 1, 1, None, 0, buf.data_ptr(),
                  lib.current_stream_ptr(DEV)) == 0
        torch.cuda.synchronize()
        assert _guard_ok(buf, 0)


# ----------------------------------------------------------------------------- pools
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sign", ["signed", "negative"])
@pytest.mark.parametrize("geom", [(1, 1, 8, 2), (1, 2, 24, 1), (2, 1, 64, 1), (3, 7, 8, 2), (7, 3, 24, 1), (8, 15, 64, 2), (15, 8, 8, 1),
                                  (2, 2, 24, 3), (15, 15, 24, 1), (7, 8, 64, 1), (3, 3, 8, 1), (1, 15, 24, 1)],
                         ids=lambda g: "%dx%d_c%d_n%d" % g)
def test_maxpool3x3s2_signed_and_all_negative_planes(geom, sign, dtype_name):
    """Signed inputs and all-negative planes (the -inf start must never surface, a skipped padded tap must not count as 0),
    h, w in {1, 2, 3, 7, 8, 15} mixed; exactly F.max_pool2d(3, 2, 1)."""
    h, w, c, n = geom
    lib, L = _lib()
    dt, code = DT[dtype_name]
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(h * 16 + w + c))
    if sign == "negative":
        x = -x.abs() - 0.5
    x = x.to(dt)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    count = n * ho * wo * c
    buf = _guarded(dt, count)
    lib.check(L.ap_maxpool3x3s2_nhwc(code, xd.data_ptr(), n, h, w, c, buf.data_ptr(), lib.current_stream_ptr(DEV)), "maxpool")
    torch.cuda.synchronize()
    got = buf[:count].view(n, ho, wo, c).cpu().permute(0, 3, 1, 2)
    want = F.max_pool2d(x.float(), 3, 2, 1).to(dt)
    assert torch.equal(got, want) and _guard_ok(buf, count)
    assert bool(torch.isfinite(got.float()).all()) and (sign == "signed" or bool((got.float() < 0).all()))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("hw", [1, 2, 49, 3136])
@pytest.mark.parametrize("c", [1, 5, 64])
def test_avgpool_signed_any_channel_count(c, hw, dtype_name):
    """A sequential f32 sum of hw signed terms and one division: |got - mean| <= (hw + 2) * 2^-24 * mean(|x|)."""
    lib, L = _lib()
    dt, code = DT[dtype_name]
    n = 3
    x = torch.randn(n, hw, c, generator=torch.Generator().manual_seed(hw + c)).to(dt)
    xd = x.to(DEV)
    out = _guarded(torch.float32, n * c)
    lib.check(L.ap_avgpool_nhwc(code, xd.data_ptr(), n, hw, c, out.data_ptr(), lib.current_stream_ptr(DEV)), "avgpool")
    torch.cuda.synchronize()
    err = (out[:n * c].view(n, c).cpu().double() - x.double().mean(1)).abs()
    bound = (hw + 2) * 2.0 ** -24 * x.double().abs().mean(1)
    assert bool((err <= bound).all()) and _guard_ok(out, n * c), float((err / bound).max())


# ----------------------------------------------------------------------------- depthwise 7x7 + LayerNorm, LayerNorm rows
def _per_pixel(got, want):
    """Largest ||got - want|| / ||want|| over the last dimension (the channels of one pixel / one row)."""
    got, want = got.double(), want.double()
    return float(((got - want).norm(dim=-1) / want.norm(dim=-1).clamp_min(1e-30)).max())


def _dw_params(c, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(c, 1, 7, 7, generator=g) / 7.0
    return w, 0.1 * torch.randn(c, generator=g), 0.8 + 0.4 * torch.rand(c, generator=g), 0.1 * torch.randn(c, generator=g)


def _dw_launch(dtype_name, xd, params):
    """xd [n, h, w, c] T on the device -> out [n, h, w, c] T (a guard region behind it is checked)."""
    lib, L = _lib()
    n, h, w, c = xd.shape
    wt, b, lw, lb = params
    wd = wt.reshape(c, 49).t().contiguous().to(DEV)                              # tap-major [49][C]
    bd, lwd, lbd = b.to(DEV), lw.to(DEV), lb.to(DEV)
    buf = _guarded(xd.dtype, xd.numel())
    lib.check(L.ap_dwconv7_ln_nhwc(DT[dtype_name][1], xd.data_ptr(), n, h, w, c, wd.data_ptr(), bd.data_ptr(), lwd.data_ptr(),
                                   lbd.data_ptr(), EPS, buf.data_ptr(), lib.current_stream_ptr(DEV)), "dwconv7_ln")
    torch.cuda.synchronize()
    assert _guard_ok(buf, xd.numel())
    return buf[:xd.numel()].view(n, h, w, c)


# (c, h, w): w < one run of 4 and h <= 3 (most taps outside); one w per lanes-per-pixel value the ladder can produce
# (xt = 4, 8, 16, 32, 64, 128, 256+ -> 64, 32, 16, 8, 4, 2, 1 lanes); the multi-segment path (a row of w * c elements above
# 64 KiB: float32 c 1536 w 24 and c 512 w 100, 16-bit c 1536 w 56 -- every shape runs in every type).
DW_SHAPES = [(8, 3, 1), (16, 1, 2), (96, 2, 3), (8, 2, 5), (16, 3, 4), (96, 3, 7), (8, 2, 13), (16, 1, 30), (96, 2, 61), (8, 3, 125),
             (8, 2, 260), (1536, 2, 24), (512, 2, 100), (1536, 2, 56)]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "c%d_%dx%d" % s)
def test_dwconv7_ln_non_square_segments_and_lane_ladder(shape, dtype_name):
    """Judged per pixel against OP_TOL: a wrong pixel at a segment seam or a row border cannot hide in the tensor norm."""
    c, h, w = shape
    dt = DT[dtype_name][0]
    n = 2
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(c + 3 * h + w)).to(dt)
    params = _dw_params(c, c + w)
    wt, b, lw, lb = params
    y = F.conv2d(x.double(), wt.double(), b.double(), padding=3, groups=c).to(dt).double()      # the conv output is rounded to T
    want = F.layer_norm(y.permute(0, 2, 3, 1), (c,), lw.double(), lb.double(), EPS)
    got = _dw_launch(dtype_name, x.permute(0, 2, 3, 1).contiguous().to(DEV), params).float().cpu()
    worst = _per_pixel(got, want)
    print(f"DWCONV {shape} {dtype_name}: worst pixel {worst:.2e}")
    assert worst <= OP_TOL[dtype_name], worst


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("shape", [(96, 3, 7), (512, 2, 100), (8, 2, 260)], ids=lambda s: "c%d_%dx%d" % s)
def test_dwconv7_ln_batch_equals_single_images_bit_for_bit(shape, dtype_name):
    c, h, w = shape
    dt = DT[dtype_name][0]
    x = torch.randn(3, h, w, c, generator=torch.Generator().manual_seed(c + w)).to(dt).to(DEV)
    params = _dw_params(c, c)
    whole = _dw_launch(dtype_name, x, params)
    for i in range(3):
        assert _bytes_equal(whole[i], _dw_launch(dtype_name, x[i:i + 1].contiguous(), params)[0]), i


def test_dwconv7_ln_refuses_in_place():
    lib, L = _lib()
    x = torch.full((1 * 4 * 4 * 8,), SENT, dtype=torch.float32, device=DEV)
    p = torch.zeros(49 * 8, device=DEV)
    assert L.ap_dwconv7_ln_nhwc(0, x.data_ptr(), 1, 4, 4, 8, p.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), EPS,
                                x.data_ptr(), lib.current_stream_ptr(DEV)) == lib.AP_ERR_INVALID
    assert b"dwconv7_ln_nhwc" in L.ap_last_error()
    torch.cuda.synchronize()
    assert bool((x == SENT).all())


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5])
@pytest.mark.parametrize("c", [8, 520, 4096])
def test_layernorm_rows_row_tails_and_wrapping_lanes(c, rows, dtype_name):
    """rows around the four-rows-per-workgroup edge, c = 520 / 4096 (more than 64 chunks: the lane loop wraps), a row with
    mean 40 and standard deviation 0.5; judged per row against OP_TOL."""
    lib, L = _lib()
    dt, code = DT[dtype_name]
    g = torch.Generator().manual_seed(rows + c)
    x = 3.0 * torch.randn(max(rows, 1), c, generator=g) + 1.0
    x[0] = 40.0 + 0.5 * torch.randn(c, generator=g)
    x = x[:rows].to(dt)
    lw = 0.8 + 0.4 * torch.rand(c, generator=g)
    lb = 0.1 * torch.randn(c, generator=g)
    xd = torch.zeros(rows * c + 8, dtype=dt, device=DEV)
    xd[:rows * c] = x.reshape(-1).to(DEV)
    lwd, lbd = lw.to(DEV), lb.to(DEV)
    buf = _guarded(dt, rows * c)
    lib.check(L.ap_layernorm_rows(code, xd.data_ptr(), rows, c, lwd.data_ptr(), lbd.data_ptr(), EPS, buf.data_ptr(),
                                  lib.current_stream_ptr(DEV)), "layernorm_rows")
    torch.cuda.synchronize()
    assert _guard_ok(buf, rows * c)
    if rows:
        want = F.layer_norm(x.double(), (c,), lw.double(), lb.double(), EPS)
        worst = _per_pixel(buf[:rows * c].view(rows, c).float().cpu(), want)
        print(f"LAYERNORM_ROWS rows={rows} c={c} {dtype_name}: worst row {worst:.2e}")
        assert worst <= OP_TOL[dtype_name], worst
