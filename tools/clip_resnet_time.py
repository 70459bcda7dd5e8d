#!/usr/bin/env python3
"""OpenAI CLIP ResNet encoders on the HIP kernels: kernel-only tiles/s (HIP events after warm-up) at the arch's device batch,
the per-kind profile split (stem / conv1x1 / conv3x3 / avgpool / head) with the average pools' share of the forward, the shader
clock over the timed region, and as a calibration line torch's own eager float16 channels_last forward of the tests'
restatement (tests/clip_resnet_reference.py, BatchNorm folded) on the same GPU.

    python tools/clip_resnet_time.py [--archs clip_rn50,clip_rn50x4] [--batch N] [--dtype float16] [--iters 10]
                                     [--json OUT.json] [--no-torch]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from atlaspatch_amd.encoders.clip_resnet import (ARCHS, MAX_BATCH, OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, HipClipResNet, fold_batchnorm,
                                                 random_canonical_state_dict)
from atlaspatch_amd.utils.telemetry import ClockProbe
from tests import clip_resnet_reference as ref


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
    ap.add_argument("--archs", default=",".join(ARCHS))
    ap.add_argument("--batch", type=int, default=0, help="device batch (default: the arch's MAX_BATCH)")
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16", "float32"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dt = getattr(torch, args.dtype)
    dev = torch.device("cuda:0")
    results = []
    for arch in args.archs.split(","):
        spec = ARCHS[arch]
        size, n = spec["image_size"], args.batch or MAX_BATCH[arch]
        folded = fold_batchnorm(random_canonical_state_dict(arch, 0), arch=arch, dtype=dt)
        net = HipClipResNet(arch, folded, device=dev, dtype=dt)
        tiles = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, device=dev)
        out = torch.empty((n, net.embed_dim), dtype=torch.float32, device=dev)
        fwd = lambda: net.forward_u8(tiles, OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, out)
        for _ in range(2):
            fwd()
        torch.cuda.synchronize()
        probe = ClockProbe(dev)
        probe.start()
        ms = time_events(fwd, args.iters)
        probe.stop()
        torch.cuda.synchronize()
        clock = probe.read()
        net.profile(True)
        fwd()
        prof = net.profile_read()
        net.profile(False)
        total = sum(v[0] for v in prof.values())
        row = {"arch": arch, "dtype": args.dtype, "batch": n, "image_size": size, "ms": round(ms, 3),
               "tiles_per_s": round(n / (ms * 1e-3), 1), "shader_clock_GHz": clock.get("shader_clock_GHz"),
               "workspace_GB": round(net._workspace.numel() / 1e9, 3),
               "profile_ms": {k: round(v[0], 3) for k, v in prof.items()},
               "profile_launches": {k: v[1] for k, v in prof.items()},
               "avgpool_share": round(prof["avgpool"][0] / total, 4) if total > 0 else None}
        net.release()
        if not args.no_torch:
            tw = {k: v.to(dev, dt) for k, v in folded.items()}
            tw = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in tw.items()}
            x = ((tiles.float() / 255.0 - torch.tensor(OPENAI_CLIP_MEAN, device=dev)) /
                 torch.tensor(OPENAI_CLIP_STD, device=dev)).permute(0, 3, 1, 2).to(dt).contiguous(memory_format=torch.channels_last)
            with torch.inference_mode():
                tf = lambda: ref.forward_folded(tw, x, depths=spec["depths"])
                for _ in range(2):
                    tf()
                torch.cuda.synchronize()
                tms = time_events(tf, max(1, args.iters // 2))
            row["torch_eager_ms"] = round(tms, 3)
            row["torch_eager_tiles_per_s"] = round(n / (tms * 1e-3), 1)
            del x, tw
        print(json.dumps(row), flush=True)
        results.append(row)
        del tiles, out
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(results, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
