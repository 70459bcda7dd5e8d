#!/usr/bin/env python3
"""CHIEF-CTransPath (Swin-Tiny with a convolutional stem) on the HIP kernels: kernel-only tiles/s at a stated batch (HIP events
after warm-up, 256-px tiles: device resize + preprocess + network + pool), the shader clock over the timed region, the per-kind
profile split (stem / ln / qkv / window_attn / proj / fc1 / fc2 / merge / pool), the window-attention kernel's algorithmic
bytes and achieved GB/s (and whether the batch's qkv maps fit the 256 MiB last-level cache, in which case the figure is not an
HBM fraction), and as the yardstick torch's eager forward of the same network on the same GPU: the restatement of
tests/swin_reference.py in the same dtype, with the masks and expanded bias tables cached as timm caches them.

    python tools/swin_time.py [--batches 256] [--dtype float16] [--iters 10] [--json OUT.json] [--no-torch]
"""
import argparse
import functools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from atlaspatch_amd.encoders.swin import (ARCHS, IMAGENET_MEAN, IMAGENET_STD, HipSwin, build_hip_swin_extractor,
                                          random_canonical_state_dict)
from atlaspatch_amd.utils.telemetry import ClockProbe
from tests import swin_reference as ref

HBM_MEASURED_BPS = 6.29e12   # measured HBM peak of the MI355X guides
LLC_BYTES = 256 << 20
ARCH = "chief-ctranspath"


def window_attention_bytes(spec, dsize, n, image=224):
    """Algorithmic bytes of every window-attention launch of one forward of n images: qkv read once (3C) and the output
    written once (C) per token, plus each block's f32 [heads, 49, 49] bias once; and the largest single launch's qkv bytes."""
    total, largest = 0.0, 0.0
    hw = image // 4
    for s, depth in enumerate(spec["depths"]):
        c = spec["embed_dim"] << s
        if s > 0:
            hw //= 2
        per_launch = n * hw * hw * 4 * c * dsize + spec["heads"][s] * 49 * 49 * 4
        total += depth * per_launch
        largest = max(largest, n * hw * hw * 3 * c * dsize)
    return total, largest


def time_events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256")
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16", "float32"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dt = getattr(torch, args.dtype)
    dsize = 4 if dt == torch.float32 else 2
    dev = torch.device("cuda:0")
    spec = ARCHS[ARCH]
    canonical = random_canonical_state_dict(ARCH, 0)
    batches = [int(b) for b in args.batches.split(",")]
    ex = build_hip_swin_extractor(device=dev, dtype=dt, state_dict=canonical, max_batch=max(batches))
    net: HipSwin = ex.vit
    tw = {k: v.to(dev, dt) for k, v in canonical.items()}
    # timm keeps attn_mask and the relative position index as buffers: cache what the restatement rebuilds per call
    ref.region_mask = functools.lru_cache(maxsize=None)(ref.region_mask)
    bias_cache = {}
    pair_bias = ref.pair_bias
    ref.pair_bias = lambda table: bias_cache.setdefault(table.data_ptr(), pair_bias(table).contiguous())
    probe = ClockProbe(dev)
    results = []
    for n in batches:
        tiles = torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, device=dev)
        out = torch.empty((n, net.embed_dim), dtype=torch.float32, device=dev)
        fwd = lambda: ex.extract_device(tiles, out)
        for _ in range(2):
            fwd()
        torch.cuda.synchronize()
        probe.start()
        ms = time_events(fwd, args.iters)
        probe.stop()
        torch.cuda.synchronize()
        clock = probe.read()
        net.profile(True)
        for _ in range(3):
            fwd()
        prof = net.profile_read()
        net.profile(False)
        wa_bytes, wa_largest = window_attention_bytes(spec, dsize, n)
        wa_ms = prof["window_attn"][0] / 3
        row = {"arch": ARCH, "dtype": args.dtype, "batch": n, "ms": round(ms, 3), "tiles_per_s": round(n / (ms * 1e-3), 1),
               "shader_clock_GHz": clock.get("shader_clock_GHz"),
               "profile_ms": {k: round(v[0] / 3, 3) for k, v in prof.items()},
               "profile_launches": {k: v[1] // 3 for k, v in prof.items()},
               "profile_resize_ms": round(ms - sum(v[0] for v in prof.values()) / 3, 3),
               "window_attn_mb": round(wa_bytes / 1e6, 2), "window_attn_gb_per_s": round(wa_bytes / (wa_ms * 1e-3) / 1e9, 1),
               "window_attn_share_of_measured_hbm_peak": round(wa_bytes / (wa_ms * 1e-3) / HBM_MEASURED_BPS, 4),
               "largest_qkv_map_mb": round(wa_largest / 1e6, 2), "qkv_fits_last_level_cache": bool(wa_largest <= LLC_BYTES)}
        if not args.no_torch:
            x = ((tiles[:, 16:240, 16:240].float() / 255.0 - torch.tensor(IMAGENET_MEAN, device=dev)) /
                 torch.tensor(IMAGENET_STD, device=dev)).permute(0, 3, 1, 2).to(dt).contiguous()
            with torch.inference_mode():
                tf = lambda: ref.forward(tw, x)
                for _ in range(3):
                    tf()
                torch.cuda.synchronize()
                tms = time_events(tf, args.iters)
            row["torch_eager_ms"] = round(tms, 3)
            row["torch_eager_tiles_per_s"] = round(n / (tms * 1e-3), 1)
            row["hip_over_torch"] = round(tms / ms, 3)
            del x
        print(json.dumps(row), flush=True)
        results.append(row)
        del tiles, out
        torch.cuda.empty_cache()
    ex.cleanup()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(results, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
