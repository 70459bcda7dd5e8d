"""The tile input stage and the conv-family operators on buffers beyond byte 2^31, byte 2^32 and element 2^31, through the C ABI,
and the four conv / Swin engines at a batch that puts their widest activation across element 2^31.  The cases, and the images that
straddle the lines, come from tests/far_tiles.py (tests/test_far_tiles_cpu.py holds that table to what the registered caps
reach); the checks are those of tests/far_checks.py, which the same CPU file tests on operators whose offsets wrap.

Every operator case runs its operator once on the whole far problem and checks

  A  every image, bit for bit: the problem is walked in chunks of whole images, each chunk's operands are copied into a scratch
     below 2^30 bytes, the same operator runs there and must give the far output's rows (torch.equal on the device).  None of
     these operators lets an image depend on another;
  B  sampled images against the operator's existing reference under its unchanged bound: the first image, the image that owns
     the element at each line of each buffer, the last -- and, after a second launch with one image fewer on the same buffers
     (the tail re-poisoned), the then-last image.  Pillow (ap_resample_u8, ap_jpeg_decode_tiles), oracle/cv2_resize.py and
     oracle/cv2_restated.py (ap_cv2_resize_u8, ap_tile_content_counts), the ((x / 255) - mean) / std float32 definition
     (preprocess), tests/test_gpu_tiff.py::gather_reference, render_region, tests/helpers.py::_conv_bound_ratio and the bounds of
     tests/test_gpu_conv_generality.py / tests/test_gpu_clip_resnet.py; no constant of its own;
  C  stray and missing writes: outputs start as the poison pattern (NaN patterns; 0xFF for u8, which no u8 case here can
     produce: resizers and the gather read values in 64 .. 191, the synthetic slide's palette ends at 243, the JPEG tiles are
     checked on the host) between guard bands; afterwards the guards are intact, no pattern is left in the payload, the images
     behind the last keep it, and the inputs are bitwise what the seeded generator made -- compared on the device.

No torch call of the test touches 2^31 elements at once.  Wall time and peak allocation per case as printed (`FAR ...`) by the
first run on an MI355X: see MEASURED."""
import gc
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import far_tiles as T
from tests.far_checks import FarRun, ImageOp, Region, _pattern_count, _poison
from tests.helpers import DT, U_T, _conv_bound_ratio

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MID = dict(lo=64, hi=191)        # u8 inputs whose resampled / gathered values stay away from the 0xFF poison

# case -> (wall seconds, peak GB allocated), first run on an MI355X; never an input to a check
MEASURED = {
    "resample-fused-512-448": (0.3, 9.5),
    "resample-fused-256-1024": (0.1, 6.7),
    "resample-2pass-1024-256": (0.1, 8.0),
    "resample-2pass-250-1000": (0.2, 8.0),
    "resample-2pass-many": (0.0, 0.6),
    "cv2-copy-256-256": (0.2, 10.7),
    "cv2-quad-512-256": (0.2, 6.7),
    "cv2-area-int-768-256": (0.1, 6.0),
    "cv2-area-gen-400-256": (0.1, 7.6),
    "cv2-linear-1024-256": (0.1, 5.8),
    "cv2-cubic-256-512": (0.3, 7.5),
    "preproc-chw-1024-float16": (0.2, 5.9),
    "preproc-chw-224-float32": (0.1, 12.1),
    "preproc-chw-224-bfloat16": (0.1, 8.1),
    "preproc-patch16-1024-float16": (0.0, 5.9),
    "preproc-patch14-1024-float32": (0.0, 6.4),
    "preproc-patch16-224-float32": (0.1, 12.1),
    "preproc-patch14-224-float32": (0.1, 12.1),
    "jpeg-444-976": (0.9, 8.1),
    "jpeg-420-968": (0.4, 10.8),
    "gather-256": (0.4, 10.7),
    "synth-256": (0.1, 6.4),
    "content-1024": (0.7, 5.4),
    "content-many": (0.0, 0.0),
    "conv-1x1-far-out-f16": (0.3, 11.4),
    "conv-1x1-far-out-f32": (0.1, 11.3),
    "conv-3x3-far-x-f16": (0.1, 6.0),
    "conv-3x3-far-x-f32": (0.1, 11.3),
    "dwconv7-one-seg-f16": (0.4, 10.7),
    "dwconv7-multi-seg-f16": (0.2, 10.7),
    "dwconv7-one-seg-f32": (0.2, 19.3),
    "layernorm-rows-f16": (0.1, 10.7),
    "layernorm-rows-f32": (0.1, 19.3),
    "maxpool-f16": (0.2, 7.0),
    "maxpool-f32": (0.1, 12.3),
    "avgpool-f16": (0.1, 6.1),
    "avgpool-f32": (0.1, 10.4),
    "avgpool2x2-f16": (0.1, 7.0),
    "avgpool2x2-f32": (0.1, 12.4),
    "attnpool-tokens-f16": (0.4, 15.6),
    "window-partition-f32": (0.2, 15.3),
    "window-unpartition-f32": (0.1, 15.3),
    "window-unpartition-add-f32": (0.1, 20.9),
    "patch-merge-ln-f16": (0.1, 10.7),
    "patch-merge-ln-f32": (0.1, 19.3),
    "swin-attention-float16": (0.1, 7.3),
    "swin-attention-float32": (0.1, 13.1),
    "engine-resnet50": (0.7, 17.9),
    "engine-convnext_tiny": (0.5, 6.8),
    "engine-chief-ctranspath": (0.5, 7.9),
    "engine-clip_rn50": (0.7, 17.7),
}


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    return _lib, lib, dev, _lib.current_stream_ptr(dev)


@pytest.fixture(autouse=True)
def _free():
    yield
    gc.collect()                 # an operator and its run refer to each other: their regions go with the cycle
    torch.cuda.empty_cache()


class _Op(ImageOp):
    def __init__(self, env, case):
        self.env, self.case, self.id, self.a = env, case, case.id, dict(case.args)
        self.dev = env[2]

    def call(self, fn, *args):
        _lib, lib, _, stream = self.env
        _lib.check(getattr(lib, fn)(*args, stream), f"{fn} {self.id}")
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the resizers
class Resample(_Op):
    def __init__(self, env, case):
        super().__init__(env, case)
        from atlaspatch_amd.utils.resample import pillow_resample_tables
        h, oh = self.a["h"], self.a["oh"]
        b, k, self.ks = pillow_resample_tables(h, oh, "bicubic")
        assert T.resample_route(h, h, oh, oh, self.ks, case.n)[0] == case.path
        self.b, self.k = torch.from_numpy(np.array(b)).to(self.dev), torch.from_numpy(np.array(k)).to(self.dev)
        # the two-pass kernels' intermediate [n, h, ow, 3] (the fused kernel keeps it in LDS and must not touch tmp): guarded too
        self.tmp = Region(self.dev, torch.uint8, (case.n, h * oh * 3) if case.path == "two-pass" else (1, 64))
        self.ins, self.outs = (("src", h * h * 3, torch.uint8, MID),), (("dst", oh * oh * 3, torch.uint8),)

    def launch(self, n, ins, outs):
        h, oh = self.a["h"], self.a["oh"]
        tmp = _poison(self.tmp.t)
        self.call("ap_resample_u8", ins[0].data_ptr(), n, h, h, outs[0].data_ptr(), oh, oh, self.b.data_ptr(), self.k.data_ptr(), self.ks,
                  self.b.data_ptr(), self.k.data_ptr(), self.ks, tmp.data_ptr())
        assert self.tmp.guards_intact(), f"{self.id}: C: a guard band of tmp was written"
        # the route of THIS launch (a ragged or chunked launch of 65 535 images and fewer may take the fused kernel); the h-pass
        # resamples values of 64 .. 191: never the poison
        used = n if T.resample_route(h, h, oh, oh, self.ks, n)[0] == "two-pass" else 0
        assert _pattern_count(tmp[:used]) == 0 and _pattern_count(tmp[used:]) == tmp[used:].numel(), f"{self.id}: C: tmp beyond image {used}"

    def reference(self, i, ins, gots):
        from PIL import Image
        h, oh = self.a["h"], self.a["oh"]
        want = np.asarray(Image.fromarray(ins[0].view(h, h, 3).numpy()).resize((oh, oh), Image.BICUBIC))
        return None if np.array_equal(gots[0].view(oh, oh, 3).numpy(), want) else "differs from Pillow"


class Cv2Resize(_Op):
    def __init__(self, env, case):
        super().__init__(env, case)
        h, oh = self.a["h"], self.a["oh"]
        assert T.cv2_mode(h, h, oh, oh, self.a["interp"]) == case.path
        self.ins, self.outs = (("src", h * h * 3, torch.uint8, MID),), (("dst", oh * oh * 3, torch.uint8),)

    def launch(self, n, ins, outs):
        h, oh = self.a["h"], self.a["oh"]
        self.call("ap_cv2_resize_u8", ins[0].data_ptr(), n, h, h, outs[0].data_ptr(), oh, oh, self.a["interp"], 0)

    def reference(self, i, ins, gots):
        from oracle import cv2_resize as R
        h, oh = self.a["h"], self.a["oh"]
        want = R.resize(ins[0].view(h, h, 3).numpy(), (oh, oh), self.a["interp"])
        return None if np.array_equal(gots[0].view(oh, oh, 3).numpy(), want) else "differs from the cv2 restatement"


# ----------------------------------------------------------------------------- the preprocess
class Preproc(_Op):
    def __init__(self, env, case):
        super().__init__(env, case)
        side, crop, ps = self.a["side"], self.a["crop"], self.a["ps"]
        self.dt = DT[case.buffers[1][2]][0]
        self.top = (side - crop) // 2 // 16 * 16
        self.ld = 3 * ps * ps
        self.ins, self.outs = (("src", side * side * 3, torch.uint8, {}),), (("dst", crop * crop * 3, self.dt),)

    def launch(self, n, ins, outs):
        _lib = self.env[0]
        side, crop, ps = self.a["side"], self.a["crop"], self.a["ps"]
        head = (ins[0].data_ptr(), n, side, side, self.top, self.top, crop, crop)
        if ps:
            self.call("ap_preproc_u8hwc_to_patchrows", *head, ps, _lib.f3(MEAN), _lib.f3(STD), outs[0].data_ptr(), self.ld, _lib.torch_dtype_code(self.dt))
        else:
            self.call("ap_preproc_u8hwc_to_chw", *head, _lib.f3(MEAN), _lib.f3(STD), outs[0].data_ptr(), _lib.torch_dtype_code(self.dt))

    def reference(self, i, ins, gots):
        side, crop, ps, t = self.a["side"], self.a["crop"], self.a["ps"], self.top
        x = ins[0].view(side, side, 3)[t:t + crop, t:t + crop].permute(2, 0, 1).to(torch.float32).div(255)
        ref = x.sub(torch.tensor(MEAN).view(3, 1, 1)).div(torch.tensor(STD).view(3, 1, 1))
        if ps:
            g = crop // ps
            ref = ref.unfold(1, ps, ps).unfold(2, ps, ps).permute(1, 2, 0, 3, 4).reshape(g * g, 3 * ps * ps)
        bits = torch.int32 if self.dt == torch.float32 else torch.int16
        same = torch.equal(ref.contiguous().to(self.dt).view(-1).view(bits), gots[0].view(bits))
        return None if same else "differs from ((x / 255) - mean) / std"


# ----------------------------------------------------------------------------- JPEG decode
class Jpeg(_Op):
    KINDS = 4

    def __init__(self, env, case, folder):
        super().__init__(env, case)
        from tests import jpeg_reference as ref
        from tests import jpeg_streams as js
        side = self.a["side"]
        self.sampling = {"444": ref.S444, "420": ref.S420}[self.a["sampling"]]
        yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
        streams = []
        for k in range(self.KINDS):
            rng = np.random.default_rng(side + k)
            rgb = np.stack([127 + 45 * np.sin(xx / (9.0 + k) + c) * np.cos(yy / 11.0 - c) for c in range(3)], axis=2)
            rgb = (rgb + rng.integers(-12, 13, size=rgb.shape)).astype(np.uint8)
            streams.append(js.encode(rgb, self.sampling, 90))
        self.want = [js.pillow_rgb(s) for s in streams]
        assert all(int(w.max()) < 0xFF for w in self.want), "a decoded tile holds the poison byte"
        rc, slots = js.read_slots(env[1], js.write_files(folder, streams), side, self.sampling)
        assert rc == 0 and slots.shape[1] == case.buffers[0][1], (rc, env[1].ap_last_error())
        self.distinct = torch.from_numpy(slots).to(self.dev)
        self.ins = (("slots", slots.shape[1], torch.uint8, dict(make=self.make)),)
        self.outs = (("dst", side * side * 3, torch.uint8),)

    def kind(self, i):
        return (i * 5 + i // 3) % self.KINDS

    def make(self, g, i0, n):
        i = torch.arange(i0, i0 + n, device=self.dev)
        return self.distinct[(i * 5 + i // 3) % self.KINDS]

    def launch(self, n, ins, outs):
        self.call("ap_jpeg_decode_tiles", ins[0].data_ptr(), n, self.a["side"], self.sampling, outs[0].data_ptr())

    def reference(self, i, ins, gots):
        side = self.a["side"]
        return None if np.array_equal(gots[0].view(side, side, 3).numpy(), self.want[self.kind(i)]) else "differs from Pillow"


# ----------------------------------------------------------------------------- gather, synth, content
class Gather(_Op):
    """Patch p at (37 p mod ts, 101 p mod ts) over the cache tiles p .. p + 3 (the last ones clipped to the cache's end), every
    fifth patch clipped at its right edge, every eleventh with a missing tile."""
    G = 2

    def __init__(self, env, case):
        super().__init__(env, case)
        ts, n = self.a["ts"], case.n
        p = np.arange(n)
        plan = np.empty((n, 4 + self.G * self.G), dtype=np.int32)
        plan[:, 0], plan[:, 1] = p * 37 % ts, p * 101 % ts
        plan[:, 2], plan[:, 3] = np.where(p % 5 == 3, ts - 7, ts), np.where(p % 7 == 2, ts - 3, ts)
        plan[:, 4:] = np.minimum(p[:, None] + np.arange(4)[None], n - 1)
        plan[p % 11 == 4, 5] = -1
        self.plan = plan
        self.host, self.device = self.staged(plan)
        self.ins, self.outs = (("cache", ts * ts * 3, torch.uint8, MID),), (("dst", ts * ts * 3, torch.uint8),)

    def staged(self, plan):
        return torch.from_numpy(np.ascontiguousarray(plan)).pin_memory(), torch.empty(plan.size + 64, dtype=torch.int32, device=self.dev)

    def gather(self, tiles, m, host, device, n, out):
        ts = self.a["ts"]
        self.call("ap_gather_patches", tiles.data_ptr(), m, ts, host.data_ptr(), device.data_ptr(), n, self.G, ts, ts, out.data_ptr())

    def launch(self, n, ins, outs):
        self.gather(ins[0], ins[0].shape[0], self.host, self.device, n, outs[0])

    def alone(self, run, i0, i1, outs):
        last = min(i1 + 3, self.case.n)
        plan = self.plan[i0:i1].copy()
        plan[:, 4:] = np.where(plan[:, 4:] >= 0, plan[:, 4:] - i0, -1)
        host, device = self.staged(plan)
        self.gather(run.ins[0].t[i0:last].clone(), last - i0, host, device, i1 - i0, outs[0])

    def reference(self, i, ins, gots):
        from tests.test_gpu_tiff import gather_reference
        ts = self.a["ts"]
        last = min(i + 4, self.case.n)
        tiles = self.run.ins[0].t[i:last].cpu().view(last - i, ts, ts, 3).numpy()
        plan = self.plan[i:i + 1].copy()
        plan[:, 4:] = np.where(plan[:, 4:] >= 0, plan[:, 4:] - i, -1)
        want = gather_reference(tiles, plan, self.G, ts, ts)[0]
        return None if np.array_equal(gots[0].view(ts, ts, 3).numpy(), want) else "differs from the definition"


class Synth(_Op):
    def __init__(self, env, case):
        super().__init__(env, case)
        from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec
        self.spec = SynthSpec(width=40000, height=40000)
        self.ell = torch.from_numpy(self.spec.ellipses()).to(self.dev)
        ps = self.a["ps"]
        self.ins, self.outs = (("xy", 2, torch.int32, dict(lo=-100, hi=39900)),), (("dst", ps * ps * 3, torch.uint8),)

    def launch(self, n, ins, outs):
        s = self.spec
        self.call("ap_synth_tiles", ins[0].data_ptr(), n, self.a["ps"], 1, 0, s.width, s.height, s.seed, self.ell.data_ptr(), self.ell.shape[0],
                  outs[0].data_ptr())

    def reference(self, i, ins, gots):
        from atlaspatch_amd.core.wsi.synth_pixels import render_region
        ps = self.a["ps"]
        want = render_region(self.spec, int(ins[0][0]), int(ins[0][1]), ps, ps, 0)
        return None if np.array_equal(gots[0].view(ps, ps, 3).numpy(), want) else "differs from render_region"


class Content(_Op):
    BLACK, SAT, VALUE = 50, 15, 200

    def __init__(self, env, case):
        super().__init__(env, case)
        side = self.a["side"]
        self.ins, self.outs = (("src", side * side * 3, torch.uint8, dict(make=self.make)),), (("counts", 2, torch.int32),)

    def make(self, g, i0, n):
        """Uniform noise, dark noise and bright greys in turn: the counts differ from tile to tile."""
        side = self.a["side"]
        x = torch.randint(0, 256, (n, side * side, 3), generator=g, device=self.dev, dtype=torch.uint8)
        kind = (torch.arange(i0, i0 + n, device=self.dev) % 3).view(n, 1, 1)
        x = torch.where(kind == 1, x // 4, x)
        x = torch.where(kind == 2, 224 + x[:, :, :1] % 32, x)
        return x.view(n, -1)

    def launch(self, n, ins, outs):
        side = self.a["side"]
        self.call("ap_tile_content_counts", ins[0].data_ptr(), n, side, side, self.BLACK, self.SAT, self.VALUE, outs[0].data_ptr())

    def reference(self, i, ins, gots):
        from oracle import cv2_restated as cv2r
        side = self.a["side"]
        tile = ins[0].view(side, side, 3).numpy()
        s, v = cv2r.cvtColor_RGB2HSV_sv(tile)
        want = [int((cv2r.cvtColor_RGB2GRAY(tile) < self.BLACK).sum()), int(((s < self.SAT) & (v >= self.VALUE)).sum())]
        return None if gots[0].tolist() == want else f"counts {gots[0].tolist()}, the cv2 restatement gives {want}"


# ----------------------------------------------------------------------------- the conv family
class Conv(_Op):
    def __init__(self, env, case):
        super().__init__(env, case)
        a = self.a
        self.name = case.buffers[0][2]
        self.dt, self.code = DT[self.name]
        k, cin, cout, hw = a["k"], a["cin"], a["cout"], a["hw"]
        self.ho = hw + 2 * a["pad"] - k + 1
        g = torch.Generator().manual_seed(k * 1000 + cin + cout)
        self.w = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).to(self.dt)
        self.b = 0.1 * torch.randn(cout, generator=g)
        self.wd, self.bd = self.w.permute(0, 2, 3, 1).contiguous().to(self.dev), self.b.to(self.dev)
        self.ins = (("x", hw * hw * cin, self.dt, {}),) + ((("resid", self.ho * self.ho * cout, self.dt, {}),) if a["resid"] else ())
        self.outs = (("out", self.ho * self.ho * cout, self.dt),)

    def launch(self, n, ins, outs):
        a = self.a
        self.call("ap_conv2d_nhwc_ex" if self.case.op.endswith("_ex") else "ap_conv2d_nhwc", self.code, ins[0].data_ptr(), n, a["hw"], a["hw"],
                  a["cin"], self.wd.data_ptr(), self.bd.data_ptr(), a["cout"], a["k"], 1, a["pad"], ins[1].data_ptr() if a["resid"] else None,
                  a["act"], outs[0].data_ptr())

    def reference(self, i, ins, gots):
        a, ho = self.a, self.ho
        nchw = lambda t, s, c: t.view(1, s, s, c).permute(0, 3, 1, 2)
        ratio = _conv_bound_ratio(nchw(gots[0], ho, a["cout"]).float(), nchw(ins[0], a["hw"], a["cin"]), self.w, self.b, 1, a["pad"],
                                  nchw(ins[1], ho, a["cout"]) if a["resid"] else None, a["act"], self.name)
        return None if ratio <= 1.0 else f"max err / bound {ratio:.3f}"


class _Nhwc(_Op):
    """x T [n, h, w, c] -> one output; the operand's type is the case's."""

    def __init__(self, env, case):
        super().__init__(env, case)
        self.name = case.buffers[0][2]
        self.dt, self.code = DT[self.name]
        self.h, self.w, self.c = self.a["h"], self.a["w"], self.a["c"]
        self.ins = ((case.buffers[0][0], case.buffers[0][1], self.dt, self.filler()),)
        self.outs = tuple((role, per, DT[dt][0]) for role, per, dt in case.buffers[1:])

    def filler(self):
        return {}

    def x(self, ins):
        return ins[0].view(self.h, self.w, self.c)


class Dwconv(_Nhwc):
    def __init__(self, env, case):
        super().__init__(env, case)
        from tests.test_gpu_conv_generality import _dw_params
        self.params = _dw_params(self.c, self.c + self.w)
        wt, b, lw, lb = self.params
        self.dev_params = [wt.reshape(self.c, 49).t().contiguous().to(self.dev), b.to(self.dev), lw.to(self.dev), lb.to(self.dev)]

    def launch(self, n, ins, outs):
        from tests.test_gpu_convnext import EPS
        self.call("ap_dwconv7_ln_nhwc", self.code, ins[0].data_ptr(), n, self.h, self.w, self.c, *(p.data_ptr() for p in self.dev_params), EPS,
                  outs[0].data_ptr())

    def reference(self, i, ins, gots):
        from tests.test_gpu_conv_generality import _per_pixel
        from tests.test_gpu_convnext import EPS, OP_TOL
        wt, b, lw, lb = self.params
        x = self.x(ins).permute(2, 0, 1)[None]
        y = F.conv2d(x.double(), wt.double(), b.double(), padding=3, groups=self.c).to(self.dt).double()
        want = F.layer_norm(y.permute(0, 2, 3, 1), (self.c,), lw.double(), lb.double(), EPS)
        worst = _per_pixel(gots[0].view(1, self.h, self.w, self.c).float(), want)
        return None if worst <= OP_TOL[self.name] else f"worst pixel {worst:.2e}"


class LayernormRows(_Nhwc):
    def __init__(self, env, case):
        super().__init__(env, case)
        g = torch.Generator().manual_seed(self.c)
        self.lw, self.lb = 0.8 + 0.4 * torch.rand(self.c, generator=g), 0.1 * torch.randn(self.c, generator=g)
        self.lwd, self.lbd = self.lw.to(self.dev), self.lb.to(self.dev)

    def filler(self):
        return dict(scale=3.0, shift=1.0)

    def launch(self, n, ins, outs):
        from tests.test_gpu_convnext import EPS
        self.call("ap_layernorm_rows", self.code, ins[0].data_ptr(), n, self.c, self.lwd.data_ptr(), self.lbd.data_ptr(), EPS, outs[0].data_ptr())

    def reference(self, i, ins, gots):
        from tests.test_gpu_conv_generality import _per_pixel
        from tests.test_gpu_convnext import EPS, OP_TOL
        want = F.layer_norm(ins[0].double()[None], (self.c,), self.lw.double(), self.lb.double(), EPS)
        worst = _per_pixel(gots[0].float()[None], want)
        return None if worst <= OP_TOL[self.name] else f"worst row {worst:.2e}"


class Maxpool(_Nhwc):
    def launch(self, n, ins, outs):
        self.call("ap_maxpool3x3s2_nhwc", self.code, ins[0].data_ptr(), n, self.h, self.w, self.c, outs[0].data_ptr())

    def reference(self, i, ins, gots):
        want = F.max_pool2d(self.x(ins).permute(2, 0, 1)[None].float(), 3, 2, 1).to(self.dt)[0].permute(1, 2, 0)
        return None if torch.equal(gots[0].view(want.shape), want) else "differs from F.max_pool2d(3, 2, 1)"


class Avgpool(_Nhwc):
    def launch(self, n, ins, outs):
        self.call("ap_avgpool_nhwc", self.code, ins[0].data_ptr(), n, self.h * self.w, self.c, outs[0].data_ptr())

    def reference(self, i, ins, gots):
        hw = self.h * self.w
        x = ins[0].view(hw, self.c).double()
        err, bound = (gots[0].double() - x.mean(0)).abs(), (hw + 2) * 2.0 ** -24 * x.abs().mean(0)
        return None if bool((err <= bound).all()) else f"max err / bound {float((err / bound).max()):.3f}"


class Avgpool2x2(_Nhwc):
    def launch(self, n, ins, outs):
        self.call("ap_avgpool2x2_nhwc", self.code, ins[0].data_ptr(), n, self.h, self.w, self.c, outs[0].data_ptr())

    def reference(self, i, ins, gots):
        taps = self.x(ins).double().view(self.h // 2, 2, self.w // 2, 2, self.c)
        want = taps.mean(dim=(1, 3))
        bound = U_T[self.name] * want.abs() + 2.0 ** -22 * taps.abs().mean(dim=(1, 3))
        ratio = float(((gots[0].double().view(want.shape) - want).abs() / bound.clamp_min(1e-300)).max())
        return None if ratio <= 1.0 else f"max err / bound {ratio:.3f}"


class AttnpoolTokens(_Op):
    def __init__(self, env, case):
        super().__init__(env, case)
        hw, c = self.a["hw"], self.a["c"]
        self.name = case.buffers[0][2]
        self.dt, self.code = DT[self.name]
        self.pos = (0.1 * torch.randn(hw + 1, c, generator=torch.Generator().manual_seed(hw * 7 + c))).clamp(-0.2, 0.2)
        self.posd = self.pos.to(self.dev)
        self.ins = (("x", hw * c, self.dt, dict(make=self.make)),)
        self.outs = (("tokens", (hw + 1) * c, self.dt), ("q_rows", c, self.dt))

    def make(self, g, i0, n):
        """|x| >= 0.25, so that |x + pos| >= 0.05: the relative bound of tests/test_gpu_clip_resnet.py needs normal numbers."""
        r = torch.randn(n, self.a["hw"] * self.a["c"], generator=g, device=self.dev)
        return (torch.sign(r) * (0.25 + r.abs())).to(self.dt)

    def launch(self, n, ins, outs):
        self.call("ap_clip_attnpool_tokens", self.code, ins[0].data_ptr(), self.posd.data_ptr(), n, self.a["hw"], self.a["c"], outs[0].data_ptr(),
                  outs[1].data_ptr())

    def reference(self, i, ins, gots):
        hw, c = self.a["hw"], self.a["c"]
        x64, p64, got = ins[0].view(hw, c).double(), self.pos.double(), gots[0].view(hw + 1, c)
        want0 = x64.mean(0) + p64[0]
        r0 = float(((got[0].double() - want0).abs() / (U_T[self.name] * want0.abs() + hw * 2.0 ** -24 * x64.abs().mean(0))).max())
        want = x64 + p64[1:]
        rest = float(((got[1:].double() - want).abs() / (U_T[self.name] * want.abs())).max())
        bits = torch.int32 if self.dt == torch.float32 else torch.int16
        if not torch.equal(gots[1].view(bits), got[0].contiguous().view(bits)):
            return "q_rows is not row 0"
        return None if r0 <= 1.0 and rest <= 1.0 else f"max err / bound: row 0 {r0:.3f}, rows 1.. {rest:.3f}"


# ----------------------------------------------------------------------------- the Swin operators
class Window(_Op):
    """ap_window_partition / ap_window_unpartition / ap_window_unpartition_add against pad, view and permute in torch (exact)."""

    def __init__(self, env, case):
        super().__init__(env, case)
        *ins, out = case.buffers
        self.ins = tuple((role, per, torch.float32, {}) for role, per, _ in ins)
        self.outs = ((out[0], out[1], torch.float32),)

    def launch(self, n, ins, outs):
        a = self.a
        self.call(self.case.op, *(t.data_ptr() for t in ins), n, a["h"], a["w"], a["c"], a["ws"], outs[0].data_ptr())

    def reference(self, i, ins, gots):
        h, w, c, ws = (self.a[k] for k in ("h", "w", "c", "ws"))
        ny, nx = -(-h // ws), -(-w // ws)
        if self.case.op == "ap_window_partition":
            x = F.pad(ins[0].view(h, w, c), (0, 0, 0, nx * ws - w, 0, ny * ws - h))
            want = x.view(ny, ws, nx, ws, c).permute(0, 2, 1, 3, 4).reshape(-1)
        else:
            want = ins[0].view(ny, nx, ws, ws, c).permute(0, 2, 1, 3, 4).reshape(ny * ws, nx * ws, c)[:h, :w].reshape(-1)
            if len(ins) == 2:
                want = ins[1] + want
        return None if torch.equal(gots[0], want) else "differs from the torch formulation"


class PatchMerge(_Nhwc):
    def __init__(self, env, case):
        super().__init__(env, case)
        g = torch.Generator().manual_seed(self.c)
        self.gamma, self.beta = torch.randn(4 * self.c, generator=g) * 0.5 + 1.0, torch.randn(4 * self.c, generator=g) * 0.3
        self.gd, self.bd = self.gamma.to(self.dev), self.beta.to(self.dev)

    def filler(self):
        return dict(shift=6.0)

    def launch(self, n, ins, outs):
        from tests import swin_ops_reference as R
        self.call("ap_patch_merge_ln", self.code, ins[0].data_ptr(), n, self.h, self.w, self.c, self.gd.data_ptr(), self.bd.data_ptr(), R.LN_EPS,
                  outs[0].data_ptr())

    def reference(self, i, ins, gots):
        from tests import swin_ops_reference as R
        a = dict(dtype=self.dt, x=ins[0].view(1, self.h, self.w, self.c), n=1, h=self.h, w=self.w, c=self.c, eps=R.LN_EPS, gamma=self.gamma,
                 beta=self.beta)
        want = R.ref_patch_merge_ln(a)["out"]
        bad = R.failures(gots[0].view(1, self.h // 2, self.w // 2, 4 * self.c), want, R.k_of("patch_merge_ln", want))
        return f"{bad} elements beyond the bound" if bad else None


class SwinAttention(_Op):
    def __init__(self, env, case):
        super().__init__(env, case)
        from atlaspatch_amd.encoders.swin import expand_relative_bias
        h, heads = self.a["h"], self.a["heads"]
        self.name = case.buffers[0][2]
        self.dt, self.code = DT[self.name]
        self.bias = expand_relative_bias(torch.randn(169, heads, generator=torch.Generator().manual_seed(heads)))
        self.biasd = self.bias.to(self.dev)
        self.ins, self.outs = (("qkv", h * h * 3 * heads * 32, self.dt, {}),), (("out", h * h * heads * 32, self.dt),)

    def launch(self, n, ins, outs):
        h, heads = self.a["h"], self.a["heads"]
        self.call("ap_swin_window_attention", self.code, ins[0].data_ptr(), n, h, h, heads, self.a["shift"], self.biasd.data_ptr(), outs[0].data_ptr())

    def reference(self, i, ins, gots):
        from tests import swin_ops_reference as R
        h, heads = self.a["h"], self.a["heads"]
        a = dict(dtype=self.dt, qkv=ins[0].view(1, h, h, 3 * heads * 32), bias=self.bias, n=1, h=h, w=h, heads=heads, shift=self.a["shift"])
        want = R.ref_window_attention(a)["out"]
        bad = R.failures(gots[0].view(1, h, h, heads * 32), want, R.k_of("window_attention", want))
        return f"{bad} elements beyond the bound" if bad else None


OPS = {"ap_window_partition": Window, "ap_window_unpartition": Window, "ap_window_unpartition_add": Window, "ap_patch_merge_ln": PatchMerge,
       "ap_swin_window_attention": SwinAttention, "ap_resample_u8": Resample, "ap_cv2_resize_u8": Cv2Resize, "ap_preproc_u8hwc_to_chw": Preproc, "ap_preproc_u8hwc_to_patchrows": Preproc,
       "ap_jpeg_decode_tiles": Jpeg, "ap_gather_patches": Gather, "ap_synth_tiles": Synth, "ap_tile_content_counts": Content,
       "ap_conv2d_nhwc": Conv, "ap_conv2d_nhwc_ex": Conv, "ap_dwconv7_ln_nhwc": Dwconv, "ap_layernorm_rows": LayernormRows,
       "ap_maxpool3x3s2_nhwc": Maxpool, "ap_avgpool_nhwc": Avgpool, "ap_avgpool2x2_nhwc": Avgpool2x2, "ap_clip_attnpool_tokens": AttnpoolTokens}


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in T.OP_CASES])
def test_operator_far_tiles(env, case, tmp_path):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    op = OPS[case.op](env, case, tmp_path) if case.op == "ap_jpeg_decode_tiles" else OPS[case.op](env, case)
    have = {(name, per, dt) for name, per, dt, _ in op.ins} | set(op.outs)
    assert {(role, per, getattr(torch, dt)) for role, per, dt in case.buffers if role != "tmp"} <= have, "the operator's buffers are not the table's"
    run = FarRun(op, case.n, env[2])
    op.run = run
    chunks, images = run.all_checks()
    print(f"FAR {case.id}: {case.n} images, {case.bytes() / 1e9:.2f} GB, wall {time.time() - t0:.1f} s, peak "
          f"{torch.cuda.max_memory_allocated() / 1e9:.1f} GB allocated, {chunks} chunks, images {images} (recorded {MEASURED.get(case.id)})")


# ----------------------------------------------------------------------------- refusals: tiny buffers, nothing launched
def test_documented_limits_are_refused_by_name(env):
    """Each launcher's limit on the problem size returns AP_ERR_INVALID with the limit's own message, before anything is
    launched: the outputs (a few KiB; the calls describe problems of terabytes) keep their poison."""
    _lib, lib, dev, stream = env
    big = (1 << 31) - 1
    src = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    f = torch.zeros(1 << 14, dtype=torch.float32, device=dev)
    out = Region(dev, torch.float32, (64, 64))
    o, s, p = out.t.data_ptr(), src.data_ptr(), f.data_ptr()
    mean, std = _lib.f3(MEAN), _lib.f3(STD)
    edge = 2139127680                 # x 257 pixels = 2^39 - 128: 2^31 workgroups of 256, one more than a grid holds
    assert (1 << 39) - 256 < edge * 257 < 1 << 39 and edge <= big
    calls = {
        # conv: M = n * Ho * Wo = 2^31 - 127 and 2^31 - 1 (the launcher admitted both before); then the workgroup count
        "conv2d_nhwc M": (lambda: lib.ap_conv2d_nhwc(0, p, big - 126, 1, 1, 8, p, p, 64, 1, 1, 0, None, 0, o, stream), "conv2d_nhwc: problem too large"),
        "conv2d_nhwc_ex M": (lambda: lib.ap_conv2d_nhwc_ex(0, p, big, 1, 1, 8, p, p, 32, 1, 1, 0, None, 0, o, stream),
                             "conv2d_nhwc_ex: problem too large"),
        "conv2d_nhwc grid": (lambda: lib.ap_conv2d_nhwc(0, p, big - 127, 1, 1, 8, p, p, 64 * 512, 1, 1, 0, None, 0, o, stream),
                             "conv2d_nhwc: grid too large"),
        "dwconv7_ln_nhwc": (lambda: lib.ap_dwconv7_ln_nhwc(0, p, 1 << 20, 1 << 11, 4, 8, p, p, p, p, 1e-6, o, stream), "dwconv7_ln_nhwc: grid too large"),
        "layernorm_rows": (lambda: lib.ap_layernorm_rows(0, p, big - 2, 8, p, p, 1e-6, o, stream), "too many (at most 2^31 - 4)"),
        "clip_attnpool_tokens": (lambda: lib.ap_clip_attnpool_tokens(0, p, p, 65536, 4, 8, o, o, stream), "clip_attnpool_tokens: n 65536"),
        "swin attention f32": (lambda: lib.ap_swin_window_attention(0, p, big, 4088, 4088, 1024, 3, p, o, stream), "swin_window_attention: grid too large"),
        "swin attention f16": (lambda: lib.ap_swin_window_attention(1, p, big, 4088, 4088, 1024, 3, p, o, stream), "swin_window_attention: grid too large"),
        "patch_merge_ln": (lambda: lib.ap_patch_merge_ln(0, p, big, 256, 256, 8, p, p, 1e-5, o, stream), "patch_merge_ln: grid too large"),
        "preproc chw": (lambda: lib.ap_preproc_u8hwc_to_chw(s, big, 16, 16, 0, 0, 16, 16, mean, std, o, 0, stream), "x 2 bands exceeds the grid"),
        "preproc rows": (lambda: lib.ap_preproc_u8hwc_to_patchrows(s, big, 32, 16, 0, 0, 32, 16, 16, mean, std, o, 768, 0, stream),
                         "x 2 bands exceeds the grid"),
        "resample": (lambda: lib.ap_resample_u8(s, big, 1024, 1000, o, 1024, 1000, p, p, 1, p, p, 1, o, stream), "ap_resample_u8: 2147483647 images"),
        "resample edge": (lambda: lib.ap_resample_u8(s, edge, 1, 9, o, 1, 257, p, p, 1, p, p, 1, o, stream), "-> 1 x 257 exceed the grid"),
        "cv2": (lambda: lib.ap_cv2_resize_u8(s, big, 8, 8, o, 32, 32, 1, 0, stream), "32 x 32 output pixels exceed the grid"),
        "cv2 edge": (lambda: lib.ap_cv2_resize_u8(s, edge, 8, 8, o, 1, 257, 1, 0, stream), "1 x 257 output pixels exceed the grid"),
        "jpeg": (lambda: lib.ap_jpeg_decode_tiles(s, big, 976, 1, o, stream), "bands exceeds the grid"),
        "synth": (lambda: lib.ap_synth_tiles(p, big, 1024, 1, 0, 1 << 20, 1 << 20, 1, p, 0, o, stream), "synth_tiles: too many pixels"),
        "content": (lambda: lib.ap_tile_content_counts(s, 1, 1 << 15, 1 << 15, 50, 15, 200, o, stream), "tile has 2^31 bytes or more"),
    }
    for name, (call, words) in calls.items():
        rc = call()
        message = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and words in message, (name, rc, message)
    torch.cuda.synchronize()
    assert _pattern_count(out.flat) == out.flat.numel(), "a refused call wrote"


# ----------------------------------------------------------------------------- engines
@pytest.mark.parametrize("name,dtype,n,per,side", T.ENGINE_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_engine_beyond_element_2_31(name, dtype, n, per, side):
    """A registered conv encoder (seeded random weights, full depth) forwards n tiles in one batch through ap_<engine>_forward_u8:
    its widest activation, `per` elements per image, crosses element 2^31 and byte 2^32.  The workspace is the caller's, exactly
    ap_<engine>_workspace_bytes(handle, n) bytes -- the figure tests/far_tiles.py restates -- between guard bands, and so is the
    output (tests/engine_workspace.py; the guards are compared on the device).  Poisoned with 0xFF (NaNs) and with 0x3C, the
    forward leaves all four guards intact and gives the same finite bits: nothing is read before it is written.  The same tiles
    in batches of 64 through the Python extractor give those bits too, the images that own the elements at the lines among them."""
    from atlaspatch_amd import _lib
    from atlaspatch_amd.encoders.clip_resnet import build_hip_clip_resnet_extractor
    from atlaspatch_amd.encoders.convnext import build_hip_convnext_extractor
    from atlaspatch_amd.encoders.resnet import build_hip_resnet_extractor
    from atlaspatch_amd.encoders.swin import build_hip_swin_extractor
    from tests import engine_workspace as W
    build = {"resnet50": build_hip_resnet_extractor, "convnext_tiny": build_hip_convnext_extractor, "chief-ctranspath": build_hip_swin_extractor,
             "clip_rn50": build_hip_clip_resnet_extractor}[name]
    dev, dt = torch.device("cuda:0"), DT[dtype][0]
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    ex = build(name="far_" + name, arch=name, device=dev, dtype=dt, random_init_seed=11, max_batch=64)
    enc, E = ex.vit, ex.embedding_dim
    straddling = T.engine_images(n, per, 2)
    assert straddling and all(0 <= i < n for i in straddling) and "2^32 bytes" in T.lines_crossed(n, per, dtype) and n * per > 1 << 31
    need = int(enc._fn("workspace_bytes")(enc._handle, n))
    assert need == T.engine_workspace_bytes(name, n, 2), "tests/far_tiles.py no longer restates the engine's workspace"
    g = torch.Generator(device=dev).manual_seed(6)
    tiles = torch.randint(0, 256, (n, side, side, 3), device=dev, dtype=torch.uint8, generator=g)
    assert ex.resized(tiles[:1]).shape[1:3] == (side, side), "the tile side was chosen to need no resize"
    ws, out = W.GuardedBytes(need, dev), W.GuardedBytes(n * E * 4, dev)
    assert ws.ptr() % 256 == 0 and out.ptr() % 16 == 0 and ws.nbytes == need
    got = {}
    for pattern in ("ff", "3c"):
        value = W.PATTERNS[pattern]
        ws.fill_in_steps(value)
        out.fill_in_steps(value)
        rc = enc._fn("forward_u8")(enc._handle, tiles.data_ptr(), n, side, side, _lib.f3(ex.mean), _lib.f3(ex.std), out.ptr(), ws.ptr(), need,
                                   _lib.current_stream_ptr(dev))
        _lib.check(rc, f"ap_{enc.ABI}_forward_u8")
        torch.cuda.synchronize()
        assert ws.guards_intact(value), f"{name}: a guard band of the workspace was written (poison {pattern})"
        assert out.guards_intact(value), f"{name}: a guard band of the output was written (poison {pattern})"
        got[pattern] = out.payload().clone().view(torch.int32).view(n, E)
    assert bool(torch.isfinite(got["ff"].view(torch.float32)).all())
    assert torch.equal(got["ff"], got["3c"]), f"{name}: the features depend on what the workspace held"
    del ws
    parts = torch.empty((n, E), dtype=torch.float32, device=dev)
    ex.forward_device(tiles, parts)                              # max_batch = 64: 42 / 28 forwards
    torch.cuda.synchronize()
    differ = torch.nonzero((parts.view(torch.int32) != got["ff"]).any(1)).flatten().tolist()
    ex.cleanup()
    print(f"FAR engine-{name}: {dtype} n = {n}, workspace {need / 1e9:.2f} GB, straddling images {straddling}, wall {time.time() - t0:.1f} s, peak "
          f"{torch.cuda.max_memory_allocated() / 1e9:.1f} GB allocated (recorded {MEASURED.get('engine-' + name)})")
    assert not differ, f"{name}: images {differ[:16]} differ between the batch of {n} and batches of 64"
