"""The C ABI on concurrent streams and host threads: what the library owns and keeps between calls (the split-K scratch of
ap_sgemm, the zero row of ap_gemm_split_f16_windows, the table caches, the per-thread error text, the engines' members) must not
leak from one stream's or one thread's call into another's.

Every concurrency test runs its calls once ALONE on the default stream -- that output is held to the float64 bound of the
operator's own test -- and then REPS times on two streams behind a gate (tests/stream_gate.py: all streams become runnable at the
same instant; the gate must still be shut after the last enqueue).  Each concurrent output must equal the solo output bit for
bit, every guard band must be intact and every input unchanged, and at least half of the repetitions must have overlapped on
the device by their timing events, or the test fails.

First-use state exists once per process: those scenarios run in children (tests/stream_first_use_child.py).

MEASURED on the MI355X (default 4 hardware queues).  Repetitions of 16 that overlapped / repetitions in which a job's output
differed from its solo output, first with the library as it was (one scratch per device, the zero row allocated and zeroed on the
first caller's stream), then with the per-stream scratch and the zero row inside the code object:

    test                                         before: overlapped, differed                       after
    (a) split-K against split-K                  16 / 16, both products in 16 of 16: FAILED          16 / 16, 0
    (b) stacked against batched split-K          16 / 16, stacked in 15, batched in 16: FAILED      16 / 16, 0
    (c) split-K against non-split controls       16 / 16, 0: passed                                  16 / 16, 0
    (e) one ViT handle, overlap option off / on  16 / 16, 0: passed                                  16 / 16, 0
    (f) ViT beside ResNet-18                     16 / 16, 0: passed                                  16 / 16, 0
    (g) host threads                             FAILED at the split-K product (thread 1, round 4)   passed
    zero_row                                     not failed (the fresh allocation held zeros)        passed
    growth, lut_first, attr_first                passed                                              passed

Solo outputs against float64: ViT n = 3 / 5 / 512 norm-wise 1.21e-3 / 1.03e-3 / 9.9e-4 (bound 4e-3), ResNet-18 n = 2 8.6e-4 (bound
1.05e-3), attr_first 1.64e-3 (bound 4e-3).
Seconds per test: (a) 0.9, (b) 0.8, (c) 0.8, (e) 0.8 / 1.3, (f) 1.0, (g) 0.5, the four children 2.1 to 2.6 each (process start).
Two things the first runs taught: a stream's first launch and a kernel's first launch each take longer than the gate stays shut
(stream_gate.warm, the warm-up products of the growth child).  And while the zero row was still allocated at first use and zeroed
on a stream of the library's own, the zero_row child passed in one run and failed its gate check in the next: the first call's
wait for its memset did not return while the gate was shut.  Supposed, not proven: five streams share four hardware queues, and
the library's stream sat behind the gated one.  The zero row is now memory that needs no first use at all."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import stream_gate as G
from tests.helpers import Guarded
from tests.test_gpu_sam2_ops import _sgemm_check          # ap_sgemm's element-wise float64 bound, as its own tests hold it

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 16
U = 2.0 ** -24


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    return _lib, _lib.load(), dev, _lib.current_stream_ptr(dev)


@pytest.fixture(scope="module")
def streams(env):
    return G.warm([torch.cuda.Stream(env[2]) for _ in range(3)])


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ----------------------------------------------------------------------------- jobs: one stream's work
class Job:
    """Deterministic work through the C ABI.  inputs: {name: (Guarded, the host tensor it was filled from)}; every run writes a
    fresh guarded output of ``out_shape`` (filled with a NaN pattern, or with ``out_init`` for an in-place operator);
    ``launch(out, stream_ptr)`` enqueues, ``check(host_out)`` holds the solo output to the operator's float64 bound."""

    def __init__(self, name, dev, inputs, out_shape, out_dtype, launch, check, out_init=None):
        self.name, self.dev, self.inputs, self.launch, self.check = name, dev, inputs, launch, check
        self.out_shape, self.out_dtype, self.out_init = tuple(out_shape), out_dtype, out_init
        self.solo = None

    def fresh(self):
        return Guarded(self.out_shape, self.out_dtype, self.dev, init=self.out_init)

    def run(self, out, stream_ptr):
        self.launch(out, stream_ptr)

    def run_solo(self, stream_ptr):
        """Once per job: alone on ``stream_ptr`` with the device idle before and after; checked against the reference."""
        if self.solo is None:
            torch.cuda.synchronize()
            out = self.fresh()
            self.run(out, stream_ptr)
            torch.cuda.synchronize()
            self.solo = out.cpu()
            self.check(self.solo)
        return self.solo

    def inputs_unchanged(self):
        for name, (buf, host) in self.inputs.items():
            assert same_bits(buf.cpu(), host), f"{self.name}: the input {name} was written"


def _guarded_inputs(dev, **arrays):
    out = {}
    for name, a in arrays.items():
        if a is not None:
            t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
            out[name] = (Guarded(tuple(t.shape), torch.float32, dev, init=t), t)
    return out


def sgemm_job(env, name, batch, M, N, K, w_kn, *, alpha=1.0, bias=False, act=0, resid=False, stack=0, calls=1, seed=0, large=False):
    """``calls`` identical ap_sgemm launches (ap_sgemm_stacked when ``stack``) into the slices of one output [calls, batch, M, N].
    large: every operand value in [70, 90], so that a partial sum over a K chunk of 160 is about 1e6."""
    _lib, lib, dev, _ = env
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.uniform(70.0, 90.0, s).astype(np.float32)) if large else (lambda *s: rng.standard_normal(s).astype(np.float32))
    A = draw(batch, M, K)
    W = draw(batch, K, N) if w_kn else draw(batch, N, K)
    b = draw(N) if bias else None
    r = draw(batch, M, N) if resid else None
    inputs = _guarded_inputs(dev, A=A, W=W, bias=b, resid=r)
    ptr = lambda key: inputs[key][0].ptr() if key in inputs else None
    ldw = N if w_kn else K

    def launch(out, sp):
        for c in range(calls):
            o = out.ptr() + 4 * c * batch * M * N
            if stack:
                assert batch == 1 and not w_kn and alpha == 1.0
                rc = lib.ap_sgemm_stacked(ptr("A"), K, ptr("W"), K, stack, M, N, K, ptr("bias"), act, ptr("resid"), N, o, N, sp)
            else:
                rc = lib.ap_sgemm(ptr("A"), K, M * K, ptr("W"), ldw, N * K, 1 if w_kn else 0, batch, M, N, K, C.c_float(alpha), ptr("bias"),
                                  act, ptr("resid"), N, M * N, o, N, M * N, sp)
            _lib.check(rc, name)

    def check(host):
        for c in range(1, calls):
            assert same_bits(host[c], host[0]), f"{name}: launch {c} of the solo run differs from launch 0"
        _sgemm_check(host[0].numpy(), A, W, w_kn, alpha, b, act, r)

    return Job(name, dev, inputs, (calls, batch, M, N), torch.float32, launch, check)


def sattention_job(env, name, nb, heads, tq, tk, d):
    """ap_sattention_split_f16 on packed q | k | v rows, as tests/test_gpu_ops.py::test_sattention_f32_vs_torch calls it: max
    |got - float64| <= 2e-5 on inputs of scale 1.3."""
    _lib, lib, dev, _ = env
    g = torch.Generator().manual_seed(nb * 7 + tq + tk + d)
    ld = 3 * heads * d
    rows_q, rows_k = torch.randn((nb * tq, ld), generator=g) * 1.3, torch.randn((nb * tk, ld), generator=g) * 1.3
    inputs = _guarded_inputs(dev, rows_q=rows_q.numpy(), rows_k=rows_k.numpy())
    scale = 1.0 / math.sqrt(d)

    def launch(out, sp):
        q, kv = inputs["rows_q"][0].ptr(), inputs["rows_k"][0].ptr()
        _lib.check(lib.ap_sattention_split_f16(q, ld, kv + 4 * heads * d, ld, kv + 8 * heads * d, ld, nb, heads, tq, tk, d, scale, out.ptr(),
                                               heads * d, sp), name)

    def check(host):
        q, k, v = rows_q[:, :heads * d], rows_k[:, heads * d:2 * heads * d], rows_k[:, 2 * heads * d:]
        qh = q.reshape(nb, tq, heads, d).permute(0, 2, 1, 3).double()
        kh = k.reshape(nb, tk, heads, d).permute(0, 2, 1, 3).double()
        vh = v.reshape(nb, tk, heads, d).permute(0, 2, 1, 3).double()
        ref = (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).permute(0, 2, 1, 3).reshape(nb * tq, heads * d)
        err = float((host.double() - ref).abs().max())
        assert bool(torch.isfinite(host).all()) and err <= 2e-5, err

    return Job(name, dev, inputs, (nb * tq, heads * d), torch.float32, launch, check)


def softmax_job(env, name, rows, cols):
    """ap_softmax_rows in place; the bound of tests/test_gpu_sam2_ops.py::test_softmax_rows_every_dispatch_edge."""
    _lib, lib, dev, _ = env
    x = (torch.randn((rows, cols), generator=torch.Generator().manual_seed(rows * cols)) * 3.0).contiguous()

    def launch(out, sp):
        _lib.check(lib.ap_softmax_rows(out.ptr(), cols, rows, cols, sp), name)

    def check(host):
        x64 = x.double().numpy()
        mx = x64.max(1, keepdims=True)
        e = np.exp(x64 - mx)
        ref = e / e.sum(1, keepdims=True)
        bound = ref * U * (np.abs(x64 - mx) + 16 + math.ceil(cols / 64)) + 2.0 ** -126
        err = np.abs(host.double().numpy() - ref)
        assert np.isfinite(host.numpy()).all() and (err <= bound).all(), float((err / bound).max())

    return Job(name, dev, {}, (rows, cols), torch.float32, launch, check, out_init=x)


class EngineJob(Job):
    """``ap_<abi>_forward_u8`` of ``enc`` on n tiles with a workspace of exactly the size the engine asks for between two guard
    bands (tests/engine_workspace.py) and an output of its own; mean / std as given."""

    def __init__(self, name, enc, tiles, mean, std, check):
        from tests import engine_workspace as EW
        self.enc, self.host_tiles = enc, tiles
        self.tiles = tiles.to(enc.device)
        n, h, w, _ = tiles.shape
        self.need = int(enc._fn("workspace_bytes")(enc._handle, n))
        self.ws = EW.GuardedBytes(self.need, enc.device)
        self.ws.fill(0xFF)
        fn, f3 = enc._fn("forward_u8"), (C.c_float * 3)

        def launch(out, sp):
            rc = fn(enc._handle, self.tiles.data_ptr(), n, h, w, f3(*mean), f3(*std), out.ptr(), self.ws.ptr(), self.need, sp)
            assert rc == 0, (name, rc, enc.lib.ap_last_error())

        super().__init__(name, enc.device, {}, (n, int(enc.embed_dim)), torch.float32, launch, check)

    def inputs_unchanged(self):
        assert torch.equal(self.tiles.cpu(), self.host_tiles), f"{self.name}: the tiles were written"
        damage = self.ws.damage(0xFF)
        assert not damage, (self.name, damage)


# ----------------------------------------------------------------------------- the gated run
def run_gated(env, streams, groups, what):
    """groups: one list of jobs per stream.  Solo runs first (cached on the jobs), then REPS gated repetitions.  Returns
    (one overlap flag per repetition, {job: repetitions whose output differed from the solo output}); asserts the gate, the guard
    bands and the inputs.  The caller asserts the two figures (``expect_clean``)."""
    _lib, lib, dev, stream0 = env
    assert len(groups) <= len(streams)
    for jobs in groups:
        for job in jobs:
            job.run_solo(stream0)
    flags, differ = [], {job.name: 0 for jobs in groups for job in jobs}
    for rep in range(REPS):
        outs = [[job.fresh() for job in jobs] for jobs in groups]
        torch.cuda.synchronize()
        gate = G.Gate(streams[:len(groups)], dev)
        sections = []
        for s, jobs, bufs in zip(streams, groups, outs):
            with gate.section(s) as sec:
                for job, out in zip(jobs, bufs):
                    job.run(out, s.cuda_stream)
            sections.append(sec)
        gate.close_check()
        torch.cuda.synchronize()
        flags.append(G.all_overlapped([sec.times() for sec in sections]))
        for jobs, bufs in zip(groups, outs):
            for job, out in zip(jobs, bufs):
                if not same_bits(out.cpu(), job.solo):               # .cpu() asserts the guard bands
                    differ[job.name] += 1
    for jobs in groups:
        for job in jobs:
            job.inputs_unchanged()
    print(f"STREAMS {what}: {sum(flags)} of {REPS} repetitions overlapped; repetitions that differed from the solo run: {differ}")
    return flags, differ


def expect_clean(result, what):
    flags, differ = result
    G.require_overlap(flags, what)
    assert not any(differ.values()), f"{what}: outputs under concurrency differ from the solo outputs in {differ} of {REPS} repetitions"


@pytest.fixture(scope="module")
def products(env):
    """The split-K products of the cases below, shapes from tests/test_gpu_ops.py::test_sgemm_mfma_vs_torch."""
    return {
        # 32 splits of k_chunk 128: 147 KB of partial sums per launch
        "pv": sgemm_job(env, "sgemm b8 m9 n16 k4096 nn", 8, 9, 16, 4096, True, calls=4, seed=1),
        # 7 splits of k_chunk 160 (the last one 40 long), partial sums about 1e6, GELU after the reduction; a run of 20
        "large": sgemm_job(env, "sgemm b1 m70 n50 k1000 nt gelu x20", 1, 70, 50, 1000, False, alpha=0.5, bias=True, act=1, calls=20, seed=2,
                           large=True),
        # three stacked problems of 9 rows, planned as one: 16 splits of k_chunk 128
        "stacked": sgemm_job(env, "sgemm_stacked 3x9 n256 k2048 relu resid", 1, 27, 256, 2048, False, bias=True, act=2, resid=True, stack=3,
                             calls=4, seed=3),
    }


def test_splitk_against_splitk(env, streams, products):
    """(a) Two split-K products on two streams.  Before the scratch was kept per stream both wrote their partial sums at offset 0 of
    the one buffer of the device, and each reduce kernel summed whatever lay there (MEASURED: the module docstring's table)."""
    expect_clean(run_gated(env, streams, [[products["pv"]], [products["large"]]], "split-K against split-K"), "split-K against split-K")


def test_stacked_splitk_against_batched_splitk(env, streams, products):
    """(b) ap_sgemm_stacked (the single problem's split-K plan) on one stream, the batched split-K product on the other."""
    expect_clean(run_gated(env, streams, [[products["stacked"]], [products["pv"]]], "stacked against batched split-K"),
                 "stacked against batched split-K")


def test_splitk_against_non_split_controls(env, streams, products):
    """(c) Controls: the fused attention and the row softmax own nothing between calls.  They pass with and without the per-stream
    scratch, and show that the gate and the comparison manufacture no differences."""
    controls = [sattention_job(env, "sattention_split_f16 3x3x160x256x64", 3, 3, 160, 256, 64), softmax_job(env, "softmax_rows 37x300", 37, 300)]
    expect_clean(run_gated(env, streams, [[products["pv"]], controls], "split-K against non-split controls"),
                 "split-K against non-split controls")


# ----------------------------------------------------------------------------- engines
VIT_ARCH = dict(image_size=64, patch_size=16, dim=512, depth=2, heads=2, head_dim=64, mlp_dim=512, ln_eps=1e-6, layer_scale=False)
HALF = (0.5, 0.5, 0.5)


@pytest.fixture(scope="module")
def vit(env):
    """The two-block float16 tower of tests/test_gpu_engine_workspace.py's narrow-attention cases (17 tokens) and its float64
    reference's inputs: (engine, state, arch)."""
    from atlaspatch_amd.encoders.vit import HipViT
    from tests import coca_reference as R
    state = R.select(R.full_state(VIT_ARCH, seed=61), VIT_ARCH)
    enc = HipViT(VIT_ARCH, state, device=env[2], dtype=torch.float16)
    yield enc, state
    enc.release()


def vit_job(vit, n, seed):
    from tests import coca_reference as R
    enc, state = vit
    tiles = torch.randint(0, 256, (n, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))

    def check(host):
        x = ((tiles.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5).contiguous()
        want = R.canonical_forward(state, x, VIT_ARCH).numpy()
        r = R.rel(host.numpy(), want)
        print(f"STREAMS vit solo n={n}: norm-wise {r:.3e} from float64 (bound {R.TOL[torch.float16]:.0e})")
        assert bool(torch.isfinite(host).all()) and r <= R.TOL[torch.float16], r

    return EngineJob(f"vit_forward_u8 n={n}", enc, tiles, HALF, HALF, check)


@pytest.mark.parametrize("overlap", [False, True], ids=["two_half_overlap_off", "two_half_overlap_on"])
def test_one_vit_handle_on_two_streams(env, streams, vit, overlap):
    """(e) One handle, two workspaces, two outputs, two streams.  off: n = 3 beside n = 5.  on: AP_VIT_OPT_TWO_HALF_OVERLAP with
    n = 512 (the one forward that forks onto the handle's side stream) beside n = 5 (below the option's threshold); the solo
    outputs are the option-off forwards."""
    enc, _ = vit
    jobs = [vit_job(vit, 512 if overlap else 3, 11), vit_job(vit, 5, 12)]
    for job in jobs:
        job.run_solo(env[3])
    enc.set_option("two_half_overlap", overlap)
    try:
        expect_clean(run_gated(env, streams, [[jobs[0]], [jobs[1]]], f"one ViT handle, overlap option {overlap}"), "one ViT handle")
    finally:
        torch.cuda.synchronize()
        enc.set_option("two_half_overlap", False)


def test_two_engines_on_two_streams(env, streams, vit):
    """(f) The ViT on one stream, a ResNet-18 (n = 2, float16, 256-px tiles through the engine's centre crop) on the other; the
    ResNet against tests/resnet_reference.py under tests/test_gpu_resnet.py's bound."""
    from atlaspatch_amd.encoders import resnet as E
    from tests import resnet_reference as ref
    from tests.helpers import _rel, _tiles
    from tests.test_gpu_resnet import NET_TOL
    sd = E.random_canonical_state_dict("resnet18", 3)
    tiles = _tiles(2)
    net = E.HipResNet("resnet18", E.fold_batchnorm(sd, arch="resnet18", dtype=torch.float16), device=env[2], dtype=torch.float16)

    def check(host):
        want = ref.extract_batch(sd, tiles, block="basic", depths=(2, 2, 2, 2))
        r = _rel(host.numpy(), want)
        print(f"STREAMS resnet18 solo n=2: norm-wise {r:.3e} (bound {NET_TOL[('resnet18', 'float16')]:.2e})")
        assert bool(torch.isfinite(host).all()) and r <= NET_TOL[("resnet18", "float16")], r

    try:
        job = EngineJob("resnet_forward_u8 n=2", net, torch.from_numpy(np.stack(tiles)), ref.MEAN, ref.STD, check)
        expect_clean(run_gated(env, streams, [[vit_job(vit, 3, 11)], [job]], "ViT beside ResNet-18"), "ViT beside ResNet-18")
    finally:
        net.release()


# ----------------------------------------------------------------------------- host threads
THREADS, ROUNDS = 4, 25
COORDS_KW = dict(level0_wh=(300 * 32, 200 * 32), downsamples=[1.0, 4.0, 16.0], src_mag=20, tgt_mag=20, patch_size=256, step_size=None,
                 tissue_thresh=0.01)


def _blob_mask(seed):
    """200 x 300 float {0, 1}: a dozen random discs, some with a hole."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:200, 0:300]
    mask = np.zeros((200, 300), np.float32)
    for _ in range(12):
        cy, cx, r = rng.integers(20, 180), rng.integers(20, 280), rng.integers(8, 40)
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        mask[d2 <= r * r] = 1.0
        if r > 20:
            mask[d2 <= (r // 3) ** 2] = 0.0
    return mask


def _resize_shape(i):
    """(h, w, oh, ow, interpolation) of the i-th resize: h alone makes all of them distinct."""
    return 8 + i, 16 + (i * 7) % 31, 5 + i % 13, 7 + (i * 3) % 17, 1 + i % 3


def test_host_threads(env):
    """(g) Four host threads, a stream each, 25 rounds of: ap_cv2_resize_u8 at a shape no other call uses (100 shapes: the table
    cache evicts at 64 while other threads hold entries), ap_preproc_u8hwc_to_chw with the thread's own new mean / std (first
    insertion into the table cache), contours + grid coordinates of a blob mask through utils.contours' worker stream, one split-K
    ap_sgemm, and a call refused for an argument only this thread gets wrong, whose message ap_last_error() must then return.
    Every result equals the reference computed beforehand on one thread: the NumPy restatement of cv2.resize, the float32
    normalisation formula and the coordinate oracle bit for bit, ap_sgemm's own solo output bit for bit."""
    from atlaspatch_amd.services.extraction import coords_from_mask
    from oracle import coords_oracle
    from oracle import cv2_resize as CV
    _lib, lib, dev, stream0 = env
    plan = []
    for t in range(THREADS):
        rng = np.random.default_rng(400 + t)
        p = {"resize": [], "errors": []}
        for r in range(ROUNDS):
            h, w, oh, ow, interp = _resize_shape(t * ROUNDS + r)
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            dst = torch.full((oh * ow * 3 + 32,), 0xA5, dtype=torch.uint8, device=dev)
            p["resize"].append((torch.from_numpy(img).to(dev), (h, w, oh, ow, interp), dst, CV.resize(img, (ow, oh), interp)))
        # K1: a (mean, std, type) triple no other test and no other thread uses
        mean, std = [0.3137 + 0.01 * t, 0.3771, 0.4419 - 0.01 * t], [0.2113, 0.2577 + 0.01 * t, 0.1931]
        dt = (torch.float16, torch.float32, torch.bfloat16, torch.float16)[t]
        src = rng.integers(0, 256, (2, 40, 48, 3), dtype=np.uint8)
        x = torch.from_numpy(src)[:, 3:35, 5:37, :].permute(0, 3, 1, 2).to(torch.float32).div(255)
        want = x.sub(torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)).div(torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)).to(dt)
        p["preproc"] = (torch.from_numpy(src).to(dev), mean, std, dt, want, [Guarded((2, 3, 32, 32), dt, dev) for _ in range(ROUNDS)])
        p["mask"] = _blob_mask(70 + t)
        p["coords"], _ = coords_oracle.coords_from_mask(p["mask"], **COORDS_KW)
        alone, _ = coords_from_mask(p["mask"], **COORDS_KW)
        assert len(p["coords"]) > 0 and np.array_equal(alone, p["coords"]), "single-threaded coordinates differ from the oracle"
        p["sgemm"] = sgemm_job(env, f"thread {t} sgemm", 1, 70, 50, 1000, False, alpha=0.5, bias=True, act=1, seed=500 + t)
        p["sgemm"].run_solo(stream0)
        p["sgemm_outs"] = [p["sgemm"].fresh() for _ in range(ROUNDS)]
        plan.append(p)
    bad = torch.ones(64, device=dev)
    torch.cuda.synchronize()
    barrier = threading.Barrier(THREADS)

    def work(t):
        p = plan[t]
        try:
            with torch.cuda.device(dev):
                stream = torch.cuda.Stream(dev)
                sp = stream.cuda_stream
                src, mean, std, dt, _, outs = p["preproc"]
                barrier.wait()
                for r in range(ROUNDS):
                    tile, (h, w, oh, ow, interp), dst, _ = p["resize"][r]
                    _lib.check(lib.ap_cv2_resize_u8(tile.data_ptr(), 1, h, w, dst.data_ptr() + 16, oh, ow, interp, 0, sp), "ap_cv2_resize_u8")
                    _lib.check(lib.ap_preproc_u8hwc_to_chw(src.data_ptr(), 2, 40, 48, 3, 5, 32, 32, _lib.f3(mean), _lib.f3(std), outs[r].ptr(),
                                                           _lib.torch_dtype_code(dt), sp), "ap_preproc_u8hwc_to_chw")
                    got, _ = coords_from_mask(p["mask"], **COORDS_KW)
                    if not np.array_equal(got, p["coords"]):
                        p["errors"].append(f"round {r}: coordinates differ from the single-threaded result")
                    p["sgemm"].run(p["sgemm_outs"][r], sp)
                    rc = lib.ap_sgemm(bad.data_ptr(), 4, 16, bad.data_ptr(), 4, 16, 0, 1, 4, 4, 4, C.c_float(1.0), None, 10 + t, None, 0, 0,
                                      bad.data_ptr(), 4, 16, sp)
                    msg = lib.ap_last_error()
                    if rc != _lib.AP_ERR_INVALID or f"activation {10 + t}".encode() not in msg:
                        p["errors"].append(f"round {r}: refused call gave {rc} and the message {msg!r}")
                stream.synchronize()
        except Exception as exc:                                   # reported by the main thread
            p["errors"].append(repr(exc))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    for t, p in enumerate(plan):
        assert not p["errors"], (t, p["errors"][:3])
        for r, (tile, (h, w, oh, ow, interp), dst, want) in enumerate(p["resize"]):
            host = dst.cpu().numpy()
            assert (host[:16] == 0xA5).all() and (host[16 + oh * ow * 3:] == 0xA5).all(), (t, r, "resize wrote outside its output")
            assert np.array_equal(host[16:16 + oh * ow * 3].reshape(oh, ow, 3), want), (t, r, (h, w, oh, ow, interp))
        for r, out in enumerate(p["preproc"][5]):
            assert same_bits(out.cpu(), p["preproc"][4]), (t, r, "preproc")
        for r, out in enumerate(p["sgemm_outs"]):
            assert same_bits(out.cpu(), p["sgemm"].solo), (t, r, "sgemm")
        p["sgemm"].inputs_unchanged()
    assert bool((bad == 1.0).all())


# ----------------------------------------------------------------------------- first use, in a fresh process each
@pytest.mark.parametrize("scenario", ["zero_row", "growth", "lut_first", "attr_first"])
def test_first_use_in_a_fresh_process(scenario):
    """tests/stream_first_use_child.py, one scenario per child, one child at a time; the child prints a JSON verdict."""
    proc = subprocess.run([sys.executable, "-m", "tests.stream_first_use_child", scenario], cwd=ROOT, capture_output=True, text=True,
                          timeout=120)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-2000:])
    verdict = json.loads(proc.stdout.strip().splitlines()[-1])
    print(f"STREAMS first use {scenario}: {verdict}")
    assert verdict["scenario"] == scenario and verdict["ok"], verdict
