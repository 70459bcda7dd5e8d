"""JPEG streams for the coefficient-reader and device-decoder tests, written in memory with Pillow, and the calls both test
files share.  No test of its own."""
import ctypes as C
import io

import numpy as np
from PIL import Image

from tests import jpeg_reference as ref

SIDES = (8, 16, 24, 25, 40)
SAMPLINGS = (ref.GRAY, ref.S444, ref.S422, ref.S420)
QUALITIES = (30, 75, 95)
CONTENTS = ("smooth", "noise", "mix")
_PIL_SUBSAMPLING = {ref.S444: 0, ref.S422: 1, ref.S420: 2}


def pixels(side, content, seed=0):
    """uint8 [side, side, 3]: a smooth field, uniform noise, or a smooth field with a noisy rectangle."""
    rng = np.random.default_rng(1000 * side + seed)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    smooth = np.stack([127 + 120 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], axis=2)
    smooth = np.clip(smooth + np.array([20.0, -30.0, 10.0]), 0, 255).astype(np.uint8)
    noise = rng.integers(0, 256, size=(side, side, 3), dtype=np.uint8)
    if content == "smooth":
        return smooth
    if content == "noise":
        return noise
    out = smooth.copy()
    out[side // 3:, : max(1, 2 * side // 3)] = noise[side // 3:, : max(1, 2 * side // 3)]
    return out


def encode(rgb, sampling, quality, **kw):
    img = Image.fromarray(rgb)
    if sampling == ref.GRAY:
        img = img.convert("L")
    else:
        kw["subsampling"] = _PIL_SUBSAMPLING[sampling]
    buf = io.BytesIO()
    img.save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_rgb(stream):
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def matrix(side, sampling):
    """[(label, stream)] for one side and sampling: every quality x content, then restart markers and optimised tables."""
    out = []
    for content in CONTENTS:
        rgb = pixels(side, content)
        for q in QUALITIES:
            out.append((f"{content}-q{q}", encode(rgb, sampling, q)))
        out.append((f"{content}-restart", encode(rgb, sampling, 75, restart_marker_blocks=2)))
        out.append((f"{content}-optimize", encode(rgb, sampling, 75, optimize=True)))
    return out


def write_files(folder, streams, prefix="t"):
    paths = []
    for i, s in enumerate(streams):
        p = folder / f"{prefix}{i}.jpg"
        p.write_bytes(s)
        paths.append(str(p))
    return paths


def read_slots(lib, paths, side, sampling, poison=0xA5):
    """(return code, uint8 [n, slot_bytes]) of ap_host_jpeg_coefficients on poisoned slots."""
    stride = lib.ap_jpeg_slot_bytes(side, sampling)
    assert stride == ref.slot_bytes(side, sampling)
    buf = np.full((len(paths), stride), poison, dtype=np.uint8)
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    rc = lib.ap_host_jpeg_coefficients(buf.ctypes.data, arr, len(paths), side, sampling)
    return rc, buf


def patch_sof_sampling(stream, value, component=0):
    """The stream with the frame header's sampling byte (h << 4 | v) of one component replaced."""
    sof = stream.index(b"\xff\xc0")
    at = sof + 2 + 2 + 1 + 2 + 2 + 1 + 3 * component + 1
    return stream[:at] + bytes([value]) + stream[at + 1:]


def truncate_entropy(stream, keep=0.5):
    """The stream cut inside its entropy-coded data (headers intact, no EOI)."""
    sos = stream.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(stream[sos + 2:sos + 4], "big")
    return stream[:start + int((len(stream) - 2 - start) * keep)]
