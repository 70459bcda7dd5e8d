#!/usr/bin/env python3
"""omiclip (open_clip coca_ViT-L-14 visual tower: 257 tokens) and conch_v15 (CONCH v1.5: 785 tokens) on the HIP kernels -- ViT-L
trunks of 24 blocks behind an attentional pooler with eight 96-wide heads: kernel-only tiles/s at one batch size (HIP events after
warm-up; 256-px uint8 tiles in HBM: device resize to 224 / 448 + preprocess + network + pooler), random weights, the shader clock
over the timed region and the per-kind milliseconds of ap_vit_profile_read; and, as the yardstick, the restatement of the same
network (tests/coca_reference.py: nn.MultiheadAttention on the packages' key names) in torch eager .half() on the same GPU (its
input already resized and normalised: the resize is not charged to it).  Both architectures are restated from the public packages,
unverified offline.

Each part is a program of its own, so that each can run under its own time limit; the second reads the first's JSON for the ratio:

    python tools/coca_time.py --part hip   --name omiclip --batch 64 --json OUT/hip.json
    python tools/coca_time.py --part torch --name omiclip --batch 64 --json OUT/torch.json --against OUT/hip.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from atlaspatch_amd.utils.telemetry import ClockProbe


def time_events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def part_hip(args, dev, dt):
    from atlaspatch_amd.encoders.vit import ARCHS, TRANSFORM_NORM, TRANSFORM_RESIZE, build_hip_vit_extractor
    spec = dict(ARCHS[args.name], depth=args.depth)
    mean, std = TRANSFORM_NORM[args.name]
    ex = build_hip_vit_extractor(name=args.name, arch=spec, device=dev, dtype=dt, random_init_seed=0, mean=mean, std=std,
                                 resize=TRANSFORM_RESIZE[args.name], expect_size=None, max_batch=args.batch)
    n = args.batch
    tiles = torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((n, ex.embedding_dim), dtype=torch.float32, device=dev)
    fwd = lambda: ex.extract_device(tiles, out)
    for _ in range(2):
        fwd()
    torch.cuda.synchronize()
    probe = ClockProbe(dev)
    probe.start()
    ms = time_events(fwd, args.iters)
    probe.stop()
    torch.cuda.synchronize()
    clock = probe.read()
    ex.vit.profile(True)
    for _ in range(2):
        fwd()
    prof = ex.vit.profile_read()
    ex.vit.profile(False)
    row = {"part": "hip", "arch": args.name, "depth": args.depth, "dtype": args.dtype, "batch": n, "ms": round(ms, 3),
           "tiles_per_s": round(n / (ms * 1e-3), 1), "shader_clock_GHz": clock.get("shader_clock_GHz"),
           "profile_ms": {k: round(v[0] / 2, 3) for k, v in prof.items()},
           "profile_launches": {k: v[1] // 2 for k, v in prof.items()},
           # what no kind times (the device resize, the pooler, memsets) minus what the profiling events themselves cost
           "ms_minus_profiled_ms": round(ms - sum(v[0] for v in prof.values()) / 2, 3),
           "finite": bool(torch.isfinite(out).all())}
    ex.cleanup()
    return row


def part_torch(args, dev, dt):
    from tests import coca_reference as R
    torch.manual_seed(0)
    if args.name == "omiclip":
        model = R.seed_module(R.CocaModel(layers=args.depth), 0).to(dt).to(dev)
        size, call = 224, model.encode_image
    else:
        model = R.seed_module(R.ConchV15(layers=args.depth), 0).to(dt).to(dev)
        size, call = 448, model
    n = args.batch
    x = torch.randn(n, 3, size, size, device=dev, dtype=dt)
    with torch.inference_mode():
        fwd = lambda: call(x)
        for _ in range(2):
            fwd()
        torch.cuda.synchronize()
        probe = ClockProbe(dev)
        probe.start()
        ms = time_events(fwd, args.iters)
        probe.stop()
        torch.cuda.synchronize()
    row = {"part": "torch", "model": f"tests/coca_reference.py restatement of {args.name}", "depth": args.depth, "dtype": args.dtype, "batch": n,
           "torch_eager_ms": round(ms, 3), "torch_eager_tiles_per_s": round(n / (ms * 1e-3), 1),
           "shader_clock_GHz": probe.read().get("shader_clock_GHz")}
    if args.against:
        hip = json.load(open(args.against))
        assert (hip["arch"], hip["batch"], hip["depth"], hip["dtype"]) == (args.name, n, args.depth, args.dtype), "the two parts must time the same problem"
        row["hip_ms"] = hip["ms"]
        row["hip_over_torch"] = round(ms / hip["ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["hip", "torch"])
    ap.add_argument("--name", required=True, choices=["omiclip", "conch_v15"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--against", default=None, help="the hip part's JSON: adds hip_over_torch to the torch part's row")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = getattr(torch, args.dtype)
    row = part_hip(args, dev, dt) if args.part == "hip" else part_torch(args, dev, dt)
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(row, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
