"""State that exists once per process, first used from two streams or two threads at once.  One scenario per process:

    python -m tests.stream_first_use_child {zero_row | growth | lut_first | attr_first}

tests/test_gpu_streams.py starts one child per scenario, one after another, and asserts on the JSON verdict printed last and on
exit status 0.  The jobs, the gate and the bounds are the parent module's."""
import json
import sys
import threading

import numpy as np
import torch

from tests import stream_gate as G
from tests import test_gpu_streams as T
from tests.helpers import Guarded, fill_pattern


def _env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    return _lib, _lib.load(), dev, _lib.current_stream_ptr(dev)


def _pair(env, work):
    """work(t, stream) on two threads that leave a barrier together, a stream each; returns the two results, raises the first
    exception."""
    dev = env[2]
    barrier, results, errors = threading.Barrier(2), [None, None], []

    def body(t):
        try:
            with torch.cuda.device(dev):
                stream = torch.cuda.Stream(dev)
                barrier.wait()
                results[t] = work(t, stream)
                stream.synchronize()
        except Exception as exc:
            errors.append(exc)
            barrier.abort()

    threads = [threading.Thread(target=body, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    torch.cuda.synchronize()
    return results


def zero_row(env):
    """The process's first two ap_gemm_split_f16_windows mode-1 calls: on stream A, shut behind the gate, and on stream B, open.
    Geometry (3, 30, 22, 8) of tests/test_gpu_ops.py::test_gemm_split_f16_windows_equals_partition_then_gemm: 30 x 22 is no multiple
    of the window, so the gathered operand has padding rows, which read the library's zero row.  Both outputs must equal
    ap_window_partition -> ap_gemm_split_f16 bit for bit.  Device memory is filled with a NaN pattern and released first, so that
    a zero row that is allocated but not yet zeroed has a chance of holding something else than zeros (nobody controls that).
    MEASURED with the library that allocated the row at first use and zeroed it on the first caller's stream: NOT failed (one
    run; the fresh allocation held zeros).  That defect was plain in the code and is gone whatever this scenario shows."""
    _lib, lib, dev, stream0 = env
    B, H, W, ws, Cin, Cout = 3, 30, 22, 8, 96, 288
    nwy, nwx = -(-H // ws), -(-W // ws)
    M = B * nwy * nwx * ws * ws
    g = torch.Generator().manual_seed(B * H + ws)
    Wq, bq = (torch.randn((Cout, Cin), generator=g) * 0.1).to(dev), torch.randn(Cout, generator=g).to(dev)
    Wqs = torch.empty_like(Wq)
    _lib.check(lib.ap_split_f16_weights(Wq.data_ptr(), Wqs.data_ptr(), Wq.numel(), stream0), "ap_split_f16_weights")
    xs, wants, gots = [], [], []
    for _ in range(2):
        x = torch.randn((B * H * W, Cin), generator=g)
        xg = Guarded((B * H * W, Cin), torch.float32, dev, init=x)
        win, want = torch.empty((M, Cin), device=dev), torch.empty((M, Cout), device=dev)
        _lib.check(lib.ap_window_partition(xg.ptr(), B, H, W, Cin, ws, win.data_ptr(), stream0), "ap_window_partition")
        _lib.check(lib.ap_gemm_split_f16(win.data_ptr(), Cin, Wqs.data_ptr(), M, Cout, Cin, bq.data_ptr(), 0, None, 0, want.data_ptr(), Cout,
                                         stream0), "ap_gemm_split_f16")
        torch.cuda.synchronize()
        xs.append((xg, x))
        wants.append(want.cpu())
        gots.append(Guarded((M, Cout), torch.float32, dev))
    poison = fill_pattern(torch.empty(128 << 20, dtype=torch.float32, device=dev))           # 512 MB
    torch.cuda.synchronize()
    del poison
    torch.cuda.empty_cache()
    a, b = G.warm([torch.cuda.Stream(dev), torch.cuda.Stream(dev)])

    def call(i, stream):
        _lib.check(lib.ap_gemm_split_f16_windows(xs[i][0].ptr(), Cin, Wqs.data_ptr(), M, Cout, Cin, bq.data_ptr(), 0, None, 0, gots[i].ptr(), Cout,
                                                 1, B, H, W, ws, stream.cuda_stream), "ap_gemm_split_f16_windows")

    torch.cuda.synchronize()
    gate = G.Gate([a], dev)
    call(0, a)                       # the process's first mode-1 call: the zero row is allocated here
    call(1, b)
    b.synchronize()                  # B's call has run to its end ...
    gate.close_check()               # ... while A's, and whatever A's call put on its stream before it, had not begun
    torch.cuda.synchronize()
    verdict = {"open_stream_equal": T.same_bits(gots[1].cpu(), wants[1]), "gated_stream_equal": T.same_bits(gots[0].cpu(), wants[0])}
    for xg, x in xs:
        assert T.same_bits(xg.cpu(), x)
    verdict["ok"] = verdict["open_stream_equal"] and verdict["gated_stream_equal"]
    return verdict


def growth(env):
    """The split-K scratch grows while kernels that use it are queued.  Stream A, shut behind the gate: two small split-K products
    (98 KB of partial sums) and then one of 4 MB, more than twice everything before it, on the same stream.  Stream B, open: the
    4 MB product, run to its end while A still waits.  Every output must equal the product run alone afterwards.  With one scratch
    per device this rests on the outgrown buffer staying alive; with one per stream, on that and on B not touching A's."""
    _lib, lib, dev, stream0 = env
    small = T.sgemm_job(env, "small: b1 m70 n50 k1000", 1, 70, 50, 1000, False, alpha=0.5, bias=True, act=1, calls=2, seed=2, large=True)
    big_a = T.sgemm_job(env, "large on A: b8 m64 n64 k4096", 8, 64, 64, 4096, True, seed=5)
    big_b = T.sgemm_job(env, "large on B: b8 m64 n64 k4096", 8, 64, 64, 4096, True, seed=6)
    outs = {job: job.fresh() for job in (small, big_a, big_b)}
    a, b = G.warm([torch.cuda.Stream(dev), torch.cuda.Stream(dev)])
    # the kernels' code is loaded at their first launch, which takes longer than the gate stays shut: both layouts once on the
    # default stream, as split-K products of 256 bytes of partial sums (4 splits of 4 x 4), before anything is gated
    for w_kn in (False, True):
        T.sgemm_job(env, "warm-up", 1, 4, 4, 512, w_kn, seed=4).run_solo(stream0)
    torch.cuda.synchronize()
    gate = G.Gate([a], dev)
    small.run(outs[small], a.cuda_stream)
    big_a.run(outs[big_a], a.cuda_stream)
    big_b.run(outs[big_b], b.cuda_stream)
    b.synchronize()
    gate.close_check()
    torch.cuda.synchronize()
    verdict = {}
    for job in (small, big_a, big_b):
        verdict[job.name] = T.same_bits(outs[job].cpu(), job.run_solo(stream0))          # the solo run checks the float64 bound
        job.inputs_unchanged()
    verdict["ok"] = all(verdict.values())
    return verdict


def lut_first(env):
    """Two threads, the same new (mean, std, type), the table's first use at the same time: both outputs and a third, later one
    equal ((x / 255) - mean) / std in float32, rounded once, bit for bit."""
    _lib, lib, dev, stream0 = env
    mean, std, dt = [0.2917, 0.4183, 0.3659], [0.2471, 0.1873, 0.2239], torch.float16
    src = np.random.default_rng(9).integers(0, 256, (3, 40, 48, 3), dtype=np.uint8)
    x = torch.from_numpy(src)[:, 3:35, 5:37, :].permute(0, 3, 1, 2).to(torch.float32).div(255)
    want = x.sub(torch.tensor(mean).view(1, 3, 1, 1)).div(torch.tensor(std).view(1, 3, 1, 1)).to(dt)
    d_src = torch.from_numpy(src).to(dev)
    outs = [Guarded((3, 3, 32, 32), dt, dev) for _ in range(3)]
    torch.cuda.synchronize()

    def call(i, sp):
        _lib.check(lib.ap_preproc_u8hwc_to_chw(d_src.data_ptr(), 3, 40, 48, 3, 5, 32, 32, _lib.f3(mean), _lib.f3(std), outs[i].ptr(),
                                               _lib.torch_dtype_code(dt), sp), "ap_preproc_u8hwc_to_chw")

    _pair(env, lambda t, stream: call(t, stream.cuda_stream))
    call(2, stream0)
    torch.cuda.synchronize()
    verdict = {f"call_{i}_equal": T.same_bits(outs[i].cpu(), want) for i in range(3)}
    verdict["ok"] = all(verdict.values())
    return verdict


def attr_first(env):
    """Two threads make the process's first ap_attention calls at the same time, at 197 tokens (12 heads of 64, float16, n = 2:
    the kernel that needs the dynamic-LDS attribute set before its first launch).  Both outputs equal each other bit for bit and
    lie within tests/test_gpu_ops.py::test_attention_vs_torch's 4e-3 of softmax(q k^T / 8) v."""
    _lib, lib, dev, stream0 = env
    n, tokens, heads, hd = 2, 197, 12, 64
    qkv = (torch.randn((n * tokens, 3 * heads * hd), generator=torch.Generator().manual_seed(tokens)) * 1.5).half()
    d_qkv = Guarded(tuple(qkv.shape), torch.float16, dev, init=qkv)
    outs = [Guarded((n * tokens, heads * hd), torch.float16, dev) for _ in range(2)]
    torch.cuda.synchronize()

    def call(t, stream):
        _lib.check(lib.ap_attention(_lib.AP_F16, d_qkv.ptr(), outs[t].ptr(), n, tokens, heads, hd, stream.cuda_stream), "ap_attention")

    _pair(env, call)
    got = [o.cpu() for o in outs]
    q, k, v = qkv.double().view(n, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1) @ v).permute(0, 2, 1, 3).reshape(n * tokens, heads * hd)
    errs = [float((o.double() - ref).abs().max()) for o in got]
    verdict = {"equal": T.same_bits(got[0], got[1]), "max_err": errs, "input_unchanged": T.same_bits(d_qkv.cpu(), qkv)}
    verdict["ok"] = verdict["equal"] and verdict["input_unchanged"] and all(np.isfinite(e) and e <= 4e-3 for e in errs)
    return verdict


SCENARIOS = {"zero_row": zero_row, "growth": growth, "lut_first": lut_first, "attr_first": attr_first}


def main(name):
    verdict = SCENARIOS[name](_env())
    torch.cuda.synchronize()
    print(json.dumps(dict(verdict, scenario=name)))


if __name__ == "__main__":
    main(sys.argv[1])
