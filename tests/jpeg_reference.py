"""NumPy restatement of the JPEG decode arithmetic behind ``ap_jpeg_decode_tiles`` (libjpeg's JDCT_ISLOW with fancy
upsampling), operating on a coefficient slot as ``ap_host_jpeg_coefficients`` lays it out.  Holds no test of its own:
tests/test_jpeg_coefficients_cpu.py checks it (and so the host reader) against Pillow, tests/test_gpu_jpeg.py uses the
geometry helpers.

Slot: ``uint16 quant[3][64]`` (natural order, components' own order) padded to 512 bytes, then per component
``int16 [hb][wb][64]``; ``wb x hb = ceil(downsampled size / 8)``."""
import numpy as np

GRAY, S444, S422, S420 = 0, 1, 2, 3
HEADER = 512

F0298, F0390, F0541, F0765, F0899, F1175 = 2446, 3196, 4433, 6270, 7373, 9633
F1501, F1847, F1961, F2053, F2562, F3072 = 12299, 15137, 16069, 16819, 20995, 25172


def geometry(side, sampling):
    """[(plane width, plane height, blocks wide, blocks high, byte offset)] per component, and the slot size."""
    hmax, vmax = (2 if sampling >= S422 else 1), (2 if sampling == S420 else 1)
    comps, off = [], HEADER
    for c in range(1 if sampling == GRAY else 3):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = -(-side * h // hmax), -(-side * v // vmax)
        wb, hb = -(-cw // 8), -(-ch // 8)
        comps.append((cw, ch, wb, hb, off))
        off += wb * hb * 128
    return comps, off


def slot_bytes(side, sampling):
    return geometry(side, sampling)[1]


def _idct_pass(i, s):
    """One 1-D pass along axis 0 of int32 [8, ...]."""
    i = [i[k] for k in range(8)]
    z1 = (i[2] + i[6]) * F0541
    t2 = z1 - i[6] * F1847
    t3 = z1 + i[2] * F0765
    t0 = (i[0] + i[4]) << 13
    t1 = (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * F1175
    a, b, c, d = a * F0298, b * F2053, c * F3072, d * F1501
    z1, z2 = z1 * -F0899, z2 * -F2562
    z3 = z3 * -F1961 + z5
    z4 = z4 * -F0390 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d])
    return (out + (1 << (s - 1))) >> s


def plane(slot, side, sampling, c):
    """Component c's samples, uint8 -> int32 [plane height, plane width] (cropped to the downsampled size)."""
    comps, _ = geometry(side, sampling)
    cw, ch, wb, hb, off = comps[c]
    quant = slot[c * 128:(c + 1) * 128].view(np.uint16).astype(np.int32).reshape(8, 8)
    coef = slot[off:off + wb * hb * 128].view(np.int16).astype(np.int32).reshape(hb, wb, 8, 8)
    d = coef * quant                                           # [hb, wb, row, col]
    cols = _idct_pass(np.moveaxis(d, 2, 0), 11)                # along the rows index: each column transformed
    cols = np.moveaxis(cols, 0, 2)
    rows = _idct_pass(np.moveaxis(cols, 3, 0), 18)
    px = np.clip(np.moveaxis(rows, 0, 3) + 128, 0, 255)        # [hb, wb, 8, 8]
    return px.transpose(0, 2, 1, 3).reshape(hb * 8, wb * 8)[:ch, :cw].astype(np.int32)


def _h2v1(p):
    """[h, w] -> [h, 2w]; a plane at most two samples wide is replicated (libjpeg's choice)."""
    h, w = p.shape
    if w <= 2:
        return np.repeat(p, 2, axis=1)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((h, 2 * w), dtype=np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _h2v2(p):
    h, w = p.shape
    if w <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    s = np.empty((2 * h, w), dtype=np.int32)
    s[0::2] = 3 * p + up
    s[1::2] = 3 * p + down
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * h, 2 * w), dtype=np.int32)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    out[:, 0] = (4 * s[:, 0] + 8) >> 4
    out[:, -1] = (4 * s[:, -1] + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def decode(slot, side, sampling):
    """uint8 [side, side, 3] from one slot (uint8 array of ``slot_bytes(side, sampling)`` bytes)."""
    slot = np.ascontiguousarray(np.frombuffer(slot, dtype=np.uint8) if not isinstance(slot, np.ndarray) else slot)
    assert slot.dtype == np.uint8 and slot.size == slot_bytes(side, sampling), (slot.size, slot_bytes(side, sampling))
    y = plane(slot, side, sampling, 0)
    if sampling == GRAY:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cb, cr = plane(slot, side, sampling, 1), plane(slot, side, sampling, 2)
    if sampling == S422:
        cb, cr = _h2v1(cb), _h2v1(cr)
    elif sampling == S420:
        cb, cr = _h2v2(cb), _h2v2(cr)
    cb, cr = cb[:side, :side] - 128, cr[:side, :side] - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)
