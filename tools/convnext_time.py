#!/usr/bin/env python3
"""ConvNeXt encoders on the HIP kernels: kernel-only tiles/s (HIP events after warm-up, 256-px tiles: device resize +
preprocess + network + pool), FLOP and algorithmic bytes per image computed from the layer shapes, the roofline bound, the
per-kind profile split (stem / dwconv_ln / fc1 / fc2 / downsample / pool), and as a calibration line torch's own eager
channels_last forward of the same (layer_scale-folded) network on the same GPU.

    python tools/convnext_time.py [--archs convnext_tiny] [--batches 256,512] [--dtype float16] [--iters 10]
                                  [--json OUT.json] [--no-torch]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from atlaspatch_amd.encoders.convnext import (ARCHS, IMAGENET_MEAN, IMAGENET_STD, LN_EPS, HipConvNeXt, build_hip_convnext_extractor,
                                              fold_layer_scale, random_canonical_state_dict)

PEAK_F16_FLOPS = 2.5e15      # dense f16 / bf16 MFMA (spec)
PEAK_F32_FLOPS = 157.3e12    # f32 MFMA (spec)
HBM_BPS = 8.0e12             # HBM3E (spec)


def layer_costs(arch, dsize, n, tile=256):
    """Per image: (FLOP, algorithmic bytes, {kind: (FLOP, bytes)}).  FLOP = 2 x MACs of every convolution / linear layer
    (the stem's true 3 channels; the depthwise layers 49 MACs per output).  Bytes = every activation read and written once
    in the compute type (the resize's uint8 input and output, the padded stem input, each layer's input and output, fc2's
    residual read, the LayerNorms' reads and writes, the pool) + the weights once per batch of n."""
    spec = ARCHS[arch]
    w, S, R = spec["widths"], 224, spec["resize"]
    kinds = {k: [0.0, 0.0] for k in ("stem", "dwconv_ln", "fc1", "fc2", "downsample", "pool")}
    wbytes = 0.0

    def add(kind, flop, byts):
        kinds[kind][0] += flop
        kinds[kind][1] += byts

    h = S // 4
    add("stem", 2.0 * h * h * w[0] * 3 * 16,
        tile * tile * 3 + R * R * 3 * 2 + S * S * 8 * dsize * 2 + h * h * w[0] * dsize * 3)
    wbytes += w[0] * 16 * 8 * dsize
    for s, depth in enumerate(spec["depths"]):
        c = w[s]
        if s > 0:
            cp = w[s - 1]
            ho = h // 2
            add("downsample", 2.0 * ho * ho * c * cp * 4, h * h * cp * dsize * 3 + ho * ho * c * dsize)
            wbytes += c * cp * 4 * dsize
            h = ho
        for _ in range(depth):
            add("dwconv_ln", 2.0 * h * h * c * 49, 2 * h * h * c * dsize)
            add("fc1", 2.0 * h * h * c * 4 * c, 5 * h * h * c * dsize)
            add("fc2", 2.0 * h * h * 4 * c * c, 6 * h * h * c * dsize)
            wbytes += (49 * c + 8 * c) * 4 + 8 * c * c * dsize
    add("pool", 0.0, h * h * w[3] * dsize + w[3] * 4)
    flop = sum(v[0] for v in kinds.values())
    byts = sum(v[1] for v in kinds.values()) + wbytes / n
    return flop, byts, {k: (v[0], v[1]) for k, v in kinds.items()}


def torch_forward(sd, depths, x):
    """torch eager: the same network (layer_scale folded into fc2), channels_last activations."""
    def ln2d(t, wk, bk):
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), sd[wk], sd[bk], LN_EPS).permute(0, 3, 1, 2)

    x = ln2d(F.conv2d(x, sd["features.0.0.weight"], sd["features.0.0.bias"], stride=4), "features.0.1.weight",
             "features.0.1.bias")
    for s, depth in enumerate(depths):
        if s > 0:
            d = f"features.{2 * s}."
            x = F.conv2d(ln2d(x, d + "0.weight", d + "0.bias"), sd[d + "1.weight"], sd[d + "1.bias"], stride=2)
        for j in range(depth):
            p = f"features.{2 * s + 1}.{j}."
            c = x.shape[1]
            y = F.conv2d(x, sd[p + "block.0.weight"], sd[p + "block.0.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
            y = F.layer_norm(y, (c,), sd[p + "block.2.weight"], sd[p + "block.2.bias"], LN_EPS)
            y = F.linear(F.gelu(F.linear(y, sd[p + "block.3.weight"], sd[p + "block.3.bias"])), sd[p + "block.5.weight"],
                         sd[p + "block.5.bias"])
            x = x + y.permute(0, 3, 1, 2)
    return torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)


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
    ap.add_argument("--archs", default="convnext_tiny")
    ap.add_argument("--batches", default="256,512")
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16", "float32"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dt = getattr(torch, args.dtype)
    dsize = 4 if dt == torch.float32 else 2
    peak = PEAK_F32_FLOPS if dt == torch.float32 else PEAK_F16_FLOPS
    dev = torch.device("cuda:0")
    results = []
    for arch in args.archs.split(","):
        spec = ARCHS[arch]
        canonical = random_canonical_state_dict(arch, 0)
        folded = fold_layer_scale(canonical, arch=arch, dtype=dt)
        batches = [int(b) for b in args.batches.split(",")]
        ex = build_hip_convnext_extractor(name=arch, arch=arch, device=dev, dtype=dt, state_dict=canonical,
                                          max_batch=max(batches))
        net: HipConvNeXt = ex.vit
        tw = {k: v.to(dev, dt) for k, v in folded.items()}
        tw = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in tw.items()}
        for n in batches:
            tiles = torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, device=dev)
            out = torch.empty((n, net.embed_dim), dtype=torch.float32, device=dev)
            fwd = lambda: ex.extract_device(tiles, out)
            for _ in range(2):
                fwd()
            torch.cuda.synchronize()
            ms = time_events(fwd, args.iters)
            net.profile(True)
            fwd()
            prof = net.profile_read()
            net.profile(False)
            flop, byts, by_kind = layer_costs(arch, dsize, n)
            t_flop, t_byte = flop / peak, byts / HBM_BPS
            bound = "compute" if t_flop >= t_byte else "memory"
            rate = n / (ms * 1e-3)
            roof = 1.0 / max(t_flop, t_byte)
            row = {"arch": arch, "dtype": args.dtype, "batch": n, "ms": round(ms, 3), "tiles_per_s": round(rate, 1),
                   "gflop_per_image": round(flop / 1e9, 3), "mb_per_image": round(byts / 1e6, 3),
                   "roofline_tiles_per_s": round(roof, 1), "bound": bound, "mfma_bound_tiles_per_s": round(1.0 / t_flop, 1),
                   "share_of_roofline": round(rate / roof, 4),
                   "tflops": round(rate * flop / 1e12, 1), "tb_per_s": round(rate * byts / 1e12, 2),
                   "by_kind_gflop_mb_per_image": {k: [round(v[0] / 1e9, 3), round(v[1] / 1e6, 3)] for k, v in by_kind.items()},
                   "profile_ms": {k: round(v[0], 3) for k, v in prof.items()},
                   "profile_launches": {k: v[1] for k, v in prof.items()},
                   "profile_resize_ms": round(ms - sum(v[0] for v in prof.values()), 3)}
            if not args.no_torch:
                x = ((tiles[:, 16:240, 16:240].float() / 255.0 - torch.tensor(IMAGENET_MEAN, device=dev)) /
                     torch.tensor(IMAGENET_STD, device=dev)).permute(0, 3, 1, 2).to(dt).contiguous(memory_format=torch.channels_last)
                with torch.inference_mode():
                    tf = lambda: torch_forward(tw, spec["depths"], x)
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
