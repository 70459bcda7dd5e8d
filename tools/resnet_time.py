#!/usr/bin/env python3
"""ResNet encoders on the HIP kernels: kernel-only tiles/s (HIP events after warm-up), FLOP and algorithmic bytes per image
computed from the layer shapes, the roofline bound, the per-kind profile split (stem / conv1x1 / conv3x3 / pool), and as a
calibration line torch's own eager channels_last forward of the same (BatchNorm-folded) network on the same GPU.

    python tools/resnet_time.py [--archs resnet18,resnet50] [--batches 256,512,1024] [--dtype float16] [--iters 10]
                                [--json OUT.json] [--no-torch]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from atlaspatch_amd.encoders.resnet import (ARCHS, IMAGENET_MEAN, IMAGENET_STD, HipResNet, conv_layers, fold_batchnorm,
                                            random_canonical_state_dict)

PEAK_F16_FLOPS = 2.5e15      # dense f16 / bf16 MFMA (spec)
PEAK_F32_FLOPS = 157.3e12    # f32 MFMA (spec)
HBM_BPS = 8.0e12             # HBM3E (spec)


def layer_costs(arch, dsize, n):
    """Per image: (FLOP, algorithmic bytes).  FLOP = 2 Ho Wo Cout Cin k^2 per convolution (the stem's true 3 channels);
    bytes = every activation read and written once in the compute type (convolution inputs, outputs, residual reads, pools,
    the uint8 tile and the padded stem input) + the weights once per batch of n."""
    spec = ARCHS[arch]
    flop = 0.0
    act = 256 * 256 * 3 + 224 * 224 * 8 * dsize              # preprocess: read the tile, write the NHWC-8 stem input
    wbytes = 0.0
    cur, cur_blk, next_hw = 56, None, 56
    n_conv = 3 if spec["block"] == "bottleneck" else 2
    for name, cout, cin, k, stride in conv_layers(arch):
        if name == "conv1":
            ho = 112
            flop += 2.0 * ho * ho * cout * 3 * k * k
            act += 224 * 224 * 8 * dsize + ho * ho * cout * dsize
            act += ho * ho * cout * dsize + 56 * 56 * cout * dsize        # max pool
            wbytes += cout * k * k * 8 * dsize
            continue
        blk, conv = name.rsplit(".", 1)
        if blk != cur_blk:                                                # a new block: its input is the last one's output
            cur_blk, cur = blk, next_hw
        first_stride = 2 if (blk.endswith(".0") and not blk.startswith("layer1")) else 1
        out_hw = (cur - 1) // first_stride + 1
        next_hw = out_hw
        if conv == "downsample":
            hin = cur
        elif spec["block"] == "bottleneck":
            hin = cur if conv in ("conv1", "conv2") else out_hw
        else:
            hin = cur if conv == "conv1" else out_hw
        ho = (hin - 1) // stride + 1
        flop += 2.0 * ho * ho * cout * cin * k * k
        act += hin * hin * cin * dsize + ho * ho * cout * dsize
        if conv == f"conv{n_conv}":
            act += ho * ho * cout * dsize                                 # the residual read
        wbytes += cout * k * k * cin * dsize
    c = spec["embed_dim"]
    act += 7 * 7 * c * dsize + c * 4                                      # global average pool
    return flop, act + wbytes / n


def torch_forward(folded, arch, x):
    """torch eager: the same network, BatchNorm folded, channels_last."""
    spec = ARCHS[arch]
    layers = {name: (k, stride) for name, _, _, k, stride in conv_layers(arch)}

    def conv(t, name):
        k, stride = layers[name]
        return F.conv2d(t, folded[name + ".weight"], folded[name + ".bias"], stride=stride, padding=k // 2)

    x = F.max_pool2d(F.relu(conv(x, "conv1")), 3, 2, 1)
    n_conv = 3 if spec["block"] == "bottleneck" else 2
    for s, depth in enumerate(spec["depths"]):
        for b in range(depth):
            pre = f"layer{s + 1}.{b}."
            y = x
            for i in range(1, n_conv + 1):
                y = conv(y, f"{pre}conv{i}")
                if i < n_conv:
                    y = F.relu(y)
            sc = conv(x, pre + "downsample") if pre + "downsample" in layers else x
            x = F.relu(y + sc)
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
    ap.add_argument("--archs", default="resnet18,resnet50")
    ap.add_argument("--batches", default="256,512,1024")
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
        folded = fold_batchnorm(random_canonical_state_dict(arch, 0), arch=arch, dtype=dt)
        net = HipResNet(arch, folded, device=dev, dtype=dt)
        tw = {k: v.to(dev, dt) for k, v in folded.items()}
        tw = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in tw.items()}
        for n in (int(b) for b in args.batches.split(",")):
            tiles = torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, device=dev)
            out = torch.empty((n, net.embed_dim), dtype=torch.float32, device=dev)
            fwd = lambda: net.forward_u8(tiles, IMAGENET_MEAN, IMAGENET_STD, out)
            for _ in range(2):
                fwd()
            torch.cuda.synchronize()
            ms = time_events(fwd, args.iters)
            net.profile(True)
            fwd()
            prof = net.profile_read()
            net.profile(False)
            flop, byts = layer_costs(arch, dsize, n)
            t_flop, t_byte = flop / peak, byts / HBM_BPS
            bound = "compute" if t_flop >= t_byte else "memory"
            rate = n / (ms * 1e-3)
            roof = 1.0 / max(t_flop, t_byte)
            row = {"arch": arch, "dtype": args.dtype, "batch": n, "ms": round(ms, 3), "tiles_per_s": round(rate, 1),
                   "gflop_per_image": round(flop / 1e9, 3), "mb_per_image": round(byts / 1e6, 3),
                   "roofline_tiles_per_s": round(roof, 1), "bound": bound, "share_of_roofline": round(rate / roof, 4),
                   "tflops": round(rate * flop / 1e12, 1), "tb_per_s": round(rate * byts / 1e12, 2),
                   "profile_ms": {k: round(v[0], 3) for k, v in prof.items()},
                   "profile_launches": {k: v[1] for k, v in prof.items()}}
            if not args.no_torch:
                x = ((tiles[:, 16:240, 16:240].float() / 255.0 - torch.tensor(IMAGENET_MEAN, device=dev)) /
                     torch.tensor(IMAGENET_STD, device=dev)).permute(0, 3, 1, 2).to(dt).contiguous(memory_format=torch.channels_last)
                with torch.inference_mode():
                    tf = lambda: torch_forward(tw, arch, x)
                    for _ in range(3):
                        tf()
                    torch.cuda.synchronize()
                    tms = time_events(tf, args.iters)
                row["torch_eager_ms"] = round(tms, 3)
                row["torch_eager_tiles_per_s"] = round(n / (tms * 1e-3), 1)
                del x
            print(json.dumps(row), flush=True)
            results.append(row)
            del tiles, out
            torch.cuda.empty_cache()
        net.release()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(results, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
