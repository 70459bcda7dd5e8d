"""Runs full attention on the cases of tests/vit_ops_reference.py in a process of its own and saves the outputs:

    python -m tests.attention_strip_child OUT.pt

AP_ATTN_IMPL / AP_ATTN_WAVES are read once per process, so tests/test_gpu_vit_ops.py starts this module as a child with
AP_ATTN_IMPL=strip (and AP_ATTN_WAVES=8) to reach the 16-bit register-strip kernel: the width-64 cases of at most 288 tokens in
float16 and bfloat16.  The guard bands are checked here; the parent holds the outputs against the strip kernel's bound."""
import math
import sys

import torch

from tests import vit_ops_reference as R
from tests.helpers import Guarded


def run_case(_lib, lib, dev, stream, a):
    """One case through ap_attention (scale 1 / sqrt(head_dim)) or ap_attention_scaled (any other); the output on the host,
    guard bands checked."""
    dt, hd = a["dtype"], a["hd"]
    out = Guarded((a["n"] * a["tokens"], a["heads"] * hd), dt, dev)
    qkv = a["qkv"].to(dev)
    if a["scale"] == 1.0 / math.sqrt(hd):
        _lib.check(lib.ap_attention(R.CODE[dt], qkv.data_ptr(), out.ptr(), a["n"], a["tokens"], a["heads"], hd, stream), "ap_attention")
    else:
        _lib.check(lib.ap_attention_scaled(R.CODE[dt], qkv.data_ptr(), out.ptr(), a["n"], a["tokens"], a["heads"], hd, a["scale"], stream),
                   "ap_attention_scaled")
    torch.cuda.synchronize()
    return out.cpu()


def strip_cases():
    return R.cases("attention", dtypes=R.HALF, widths=(64,), kernel="strip")


def main(path):
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    lib, stream = _lib.load(), _lib.current_stream_ptr(dev)
    torch.save({case.id: run_case(_lib, lib, dev, stream, case.args) for case in strip_cases()}, path)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
