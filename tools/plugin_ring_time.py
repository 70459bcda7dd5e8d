#!/usr/bin/env python3
"""One torch module, one synthetic slide, both ways a plugin encoder can be fed, in one process.

host   the plugin registers without ``device_transform``: ``append_features`` reads, preprocesses (PIL) and uploads tile by
       tile on the calling thread -- the only route before the device transform existed.
ring   the same plugin with ``device_transform``: decode threads, pinned tile ring, resize + normalise on the device, the
       module called on device batches (``DeviceTorchFeatureExtractor``).

The module is a small CNN defined here (four stride-2 convolutions, global mean, one linear layer; float16), the transform
``Resize(224, bicubic) -> CenterCrop(224) -> ToTensor -> Normalize``.  Coordinates are computed once; every run embeds a
fresh copy of that H5 through ``process`` with 16 decode threads.  The first run of each route warms torch's convolution
choice and the ring's buffers and is not reported; the timed figure is the wall time of ``embed_all`` (encoder build, every
tile, H5 write) ending in a device synchronise, best and median of --reps, with the shader clock over the ring runs.  By
default the ring reads tiles through the pinned ring (``ATLASPATCH_HOST_TILES=1``), as a real slide does; --device-source
lets the synthetic slide render its tiles in HBM instead.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLUGIN = '''
import torch
from atlaspatch_amd.encoders.custom import CustomEncoderComponents, register_custom_encoder
from atlaspatch_amd.encoders.device_transform import DeviceTransform


def small_cnn():
    torch.manual_seed(0)
    layers, width = [], 3
    for out in (32, 64, 128, 256):
        layers += [torch.nn.Conv2d(width, out, 3, stride=2, padding=1), torch.nn.ReLU()]
        width = out
    return torch.nn.Sequential(*layers, torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(256, 256))


def register_feature_extractors(registry, device, dtype, num_workers):
    transform = DeviceTransform(resize=224, interpolation="bicubic", crop=224, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    for name, described in (("cnn_ring", transform), ("cnn_host", None)):
        register_custom_encoder(registry=registry, name=name, embedding_dim=256, device=device, dtype=dtype, num_workers=num_workers,
                                loader=lambda d, t, described=described: CustomEncoderComponents(small_cnn(), transform.host,
                                                                                                 device_transform=described))
'''


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=30000)
    ap.add_argument("--height", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--device-source", action="store_true", help="let the synthetic slide render tiles in HBM (no pinned ring)")
    args = ap.parse_args()

    import torch
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services.feature_embedding import PatchFeatureEmbeddingService
    from atlaspatch_amd.utils.telemetry import ClockProbe
    if not torch.cuda.is_available():
        raise SystemExit("plugin_ring_time needs a HIP device: a time taken elsewhere says nothing")
    if not args.device_source:
        os.environ["ATLASPATCH_HOST_TILES"] = "1"
    dev = torch.device("cuda:0")
    probe = ClockProbe(dev)
    timed = []
    inner = PatchFeatureEmbeddingService.embed_all

    def embed_all(self, results, **kw):
        torch.cuda.synchronize(dev)
        probe.start()
        t0 = time.perf_counter()
        failures = inner(self, results, **kw)
        torch.cuda.synchronize(dev)
        seconds = time.perf_counter() - t0
        probe.stop()
        torch.cuda.synchronize(dev)
        timed.append((sum(int(r.num_patches) for r in results), seconds, probe.read().get("shader_clock_GHz"), len(failures)))
        return failures

    PatchFeatureEmbeddingService.embed_all = embed_all
    with tempfile.TemporaryDirectory() as tmp:
        slide = os.path.join(tmp, "slide.synth")
        json.dump({"width": args.width, "height": args.height, "seed": 7, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16]}, open(slide, "w"))
        plugin = os.path.join(tmp, "cnn_plugin.py")
        open(plugin, "w").write(PLUGIN)
        base = os.path.join(tmp, "coords")
        common = ["--patch-size", "256", "--target-mag", "20"]
        res = CliRunner().invoke(cli, ["segment-and-get-coords", slide, "-o", base, *common], catch_exceptions=False)
        assert res.exit_code == 0, res.output
        runs = {"host": [], "ring": []}
        for rep in range(args.reps + 1):                        # rep 0 warms up
            for route in ("host", "ring"):
                out = os.path.join(tmp, f"{route}{rep}")
                shutil.copytree(base, out)
                res = CliRunner().invoke(cli, ["process", slide, "-o", out, *common, "--feature-plugin", plugin, "--feature-extractors",
                                               f"cnn_{route}", "--feature-precision", "float16", "--feature-num-workers", str(args.workers)],
                                         catch_exceptions=False)
                assert res.exit_code == 0 and "failures: 0" in res.output, res.output
                tiles, seconds, ghz, failed = timed.pop()
                assert failed == 0 and not timed
                if rep:
                    runs[route].append((tiles, seconds, ghz))
                shutil.rmtree(out)
    report = {"tiles": runs["ring"][0][0], "slide": [args.width, args.height], "decode_threads": args.workers,
              "tile_source": "device" if args.device_source else "pinned ring", "reps": args.reps}
    for route, rows in runs.items():
        rates = [t / s for t, s, _ in rows]
        report[route] = {"tiles_per_s_best": round(max(rates), 1), "tiles_per_s_median": round(statistics.median(rates), 1),
                         "seconds": [round(s, 3) for _, s, _ in rows], "shader_clock_GHz": [g for _, _, g in rows]}
    report["ring_over_host_median"] = round(report["ring"]["tiles_per_s_median"] / report["host"]["tiles_per_s_median"], 2)
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
