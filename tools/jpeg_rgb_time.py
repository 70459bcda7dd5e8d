#!/usr/bin/env python3
"""ap_jpeg_decode_tiles_ex at AP_JPEG_RGB against AP_JPEG_444 in one run, and what an RGB-coded tile weighs on the ring.

The sibling of tools/jpeg_split_time.py for RGB-coded tiles: the same synthetic slide, the same 256-pixel tiles at quality 80, written
three times -- RGB coded (Pillow ``keep_rgb=True``, 4:4:4: what a TIFF level tagged PhotometricInterpretation 2 holds), YCbCr 4:4:4
and YCbCr 4:2:0 (the twin whose ring traffic the README quotes).

    python tools/jpeg_rgb_time.py --store DIR [--side 40000] [--tiles 2048] [--iters 50]

Builds the three stores under DIR if they are not there, then per form: mean file, payload (the unstuffed entropy-coded segment the
stream route carries) and coefficient-slot bytes per tile; and for the two 4:4:4-shaped forms the time of ap_jpeg_decode_tiles_ex on
--tiles slots in HBM -- 5 launches of warm-up, then --iters launches each between its own pair of HIP events: median, minimum,
maximum, and the shader clock over the timed region.  Prints one JSON line."""
import argparse
import concurrent.futures as futures
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import jpeg_split_time as split
from atlaspatch_amd import _lib
from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec

FORMS = {"rgb": (_lib.AP_JPEG_RGB, dict(subsampling=0, keep_rgb=True)), "444": (_lib.AP_JPEG_444, dict(subsampling=0)),
         "420": (_lib.AP_JPEG_420, dict(subsampling=2))}


def build(args):
    from PIL import Image
    spec = SynthSpec(width=args.side, height=args.side, seed=1234)
    xy = np.ascontiguousarray(split._coords(spec)[:args.tiles])
    lib = _lib.load()
    ell = np.ascontiguousarray(spec.ellipses(), dtype=np.int64)
    for form in FORMS:
        os.makedirs(os.path.join(args.store, form), exist_ok=True)
    with futures.ThreadPoolExecutor(args.workers) as pool:
        for lo in range(0, len(xy), 512):
            part = np.ascontiguousarray(xy[lo:lo + 512])
            px = np.empty((len(part), 256, 256, 3), dtype=np.uint8)
            _lib.check(lib.ap_host_synth_tiles(px.ctypes.data, part.ctypes.data, len(part), 256, 1, 0, spec.width, spec.height,
                                               spec.seed, ell.ctypes.data, ell.shape[0]), "ap_host_synth_tiles")

            def put(i):
                for form, (_, kw) in FORMS.items():
                    Image.fromarray(px[i]).save(os.path.join(args.store, form, f"{part[i, 0]}_{part[i, 1]}_256.jpg"), quality=80, **kw)
            list(pool.map(put, range(len(part))))
    np.save(os.path.join(args.store, "xy.npy"), xy)


def weights(lib, paths, sampling):
    """Mean file, payload and slot bytes per tile; the payload lengths come from the stream stager's descriptors."""
    n = len(paths)
    arr = split._char_pp(paths)
    bound, used = C.c_size_t(), C.c_size_t()
    _lib.check(lib.ap_host_jpeg_stream_bound(arr, n, C.byref(bound)), "ap_host_jpeg_stream_bound")
    descs = np.zeros(n * 2048 + 16, dtype=np.uint8)
    arena = np.zeros(n * bound.value + 16, dtype=np.uint8)
    d0, a0 = (-descs.ctypes.data) % 16, (-arena.ctypes.data) % 16
    _lib.check(lib.ap_host_jpeg_streams(descs.ctypes.data + d0, arena.ctypes.data + a0, n * bound.value, C.byref(used), arr, n, 256, sampling),
               "ap_host_jpeg_streams")
    payload = descs[d0:d0 + n * 2048].reshape(n, 2048)[:, 1484:1488].copy().view(np.uint32)
    return {"mean_file_bytes": int(np.mean([os.path.getsize(p) for p in paths])), "mean_payload_bytes": int(payload.mean()),
            "slot_bytes": int(lib.ap_jpeg_slot_bytes_ex(256, sampling))}


def device(lib, paths, sampling, iters):
    import torch
    from PIL import Image
    from atlaspatch_amd.utils.telemetry import ClockProbe
    dev = torch.device("cuda:0")
    n, stride = len(paths), lib.ap_jpeg_slot_bytes_ex(256, sampling)
    host = torch.empty((n, stride), dtype=torch.uint8, pin_memory=True)
    _lib.check(lib.ap_host_jpeg_coefficients(host.data_ptr(), split._char_pp(paths), n, 256, sampling), "ap_host_jpeg_coefficients")
    slots = host.to(dev)
    rgb = torch.empty((n, 256, 256, 3), dtype=torch.uint8, device=dev)
    run = lambda: _lib.check(lib.ap_jpeg_decode_tiles_ex(slots.data_ptr(), n, 256, sampling, rgb.data_ptr(), _lib.current_stream_ptr(dev)),
                             "ap_jpeg_decode_tiles_ex")
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    probe = ClockProbe(dev)
    probe.start()
    for e0, e1 in events:
        e0.record()
        run()
        e1.record()
    torch.cuda.synchronize()
    probe.stop()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in events])
    check = all(np.array_equal(rgb[i].cpu().numpy(), np.asarray(Image.open(paths[i]).convert("RGB"))) for i in (0, n // 2, n - 1))
    moved = n * (stride + 256 * 256 * 3)
    return {"tiles": n, "launches": iters, "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
            "ms_max": round(float(ms.max()), 4), "TBs_at_median": round(moved / (float(np.median(ms)) * 1e-3) / 1e12, 3),
            "shader_clock_GHz": probe.read().get("shader_clock_GHz"), "equals_pillow": bool(check)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", required=True)
    ap.add_argument("--side", type=int, default=40000)
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.store, "xy.npy")):
        build(args)
    lib = _lib.load()
    xy = np.load(os.path.join(args.store, "xy.npy"))[:args.tiles]
    row = {"tool": "jpeg_rgb_time", "quality": 80, "side": 256}
    for form, (sampling, _) in FORMS.items():
        paths = [os.path.join(args.store, form, f"{x}_{y}_256.jpg") for x, y in xy]
        row[form] = weights(lib, paths, sampling)
        if form != "420" and split._have_gpu():
            row[form].update(device(lib, paths, sampling, args.iters))
    print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(row, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
