"""Tiled-JPEG TIFF fixtures for the native TIFF reader's tests, generated at test time (no committed binaries).

Every tile is encoded by Pillow (quality 80, chosen subsampling); the DQT / DHT segments can be moved into a JPEGTables stream
and stripped from the tiles (abbreviated streams, what Aperio and libtiff write); the classic or BigTIFF container, in either
byte order, is written here.  Edge tiles are stored full size, padded with a loud colour that must never show in a patch.
The oracle is Pillow reading the same file (``pillow_rgb``).
"""
import io
import struct

import numpy as np
from PIL import Image

SUBSAMPLING = {"gray": None, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
_YCBCR_SUB = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
PAD = (255, 0, 255)
BYTE, ASCII, SHORT, LONG, RATIONAL, UNDEFINED, LONG8 = 1, 2, 3, 4, 5, 7, 16
_SIZE = {BYTE: 1, ASCII: 1, SHORT: 2, LONG: 4, RATIONAL: 8, UNDEFINED: 1, LONG8: 8}


def image(width, height, seed=0, grey=False):
    """Smooth structure plus noise, so that chroma and luma both carry detail: uint8 [h, w, 3] (or [h, w])."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / 37.0 + seed) * np.cos(y / 23.0), 128 + 90 * np.cos(x / 11.0) * np.sin(y / 53.0 + 1),
                     128 + 110 * np.sin((x + y) / 29.0)], axis=-1)
    out = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out[..., 1]) if grey else out


def encode_tile(pixels, subsampling, *, progressive=False, quality=80):
    buf = io.BytesIO()
    if pixels.ndim == 2:
        Image.fromarray(pixels, "L").save(buf, "JPEG", quality=quality, progressive=progressive)
    else:
        Image.fromarray(pixels, "RGB").save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[subsampling], progressive=progressive)
    return buf.getvalue()


def split_tables(stream):
    """(tables-only stream, abbreviated stream): the DQT / DHT segments in front of SOS moved out."""
    assert stream[:2] == b"\xff\xd8"
    pos, tables, rest = 2, b"", b""
    while True:
        assert stream[pos] == 0xFF
        marker = stream[pos + 1]
        if marker == 0xDA:                                  # SOS: the entropy-coded data follows, copy to the end
            rest += stream[pos:]
            break
        length = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        seg = stream[pos:pos + 2 + length]
        if marker in (0xDB, 0xC4):
            tables += seg
        else:
            rest += seg
        pos += 2 + length
    return b"\xff\xd8" + tables + b"\xff\xd9", b"\xff\xd8" + rest


class _Writer:
    def __init__(self, big, be):
        self.big, self.e = big, (">" if be else "<")
        self.buf = bytearray()
        if big:
            self.buf += (b"MM" if be else b"II") + struct.pack(self.e + "HHHQ", 43, 8, 0, 0)
        else:
            self.buf += (b"MM" if be else b"II") + struct.pack(self.e + "HI", 42, 0)
        self.link = 8 if big else 4                         # where the offset of the next IFD goes
        self.value_at = {}                                  # (ifd index, tag) -> file offset of the entry's value / offset field
        self.count_at = {}
        self.next_at = []                                   # per IFD: file offset of its next-IFD pointer
        self.ifd_at = []

    def blob(self, data):
        if len(self.buf) % 2:
            self.buf += b"\0"
        off = len(self.buf)
        self.buf += data
        return off

    def pack(self, typ, values):
        if typ in (ASCII, UNDEFINED, BYTE) and isinstance(values, (bytes, bytearray)):
            return bytes(values)
        if typ == RATIONAL:
            return b"".join(struct.pack(self.e + "II", n, d) for n, d in values)
        return struct.pack(self.e + str(len(values)) + {BYTE: "B", SHORT: "H", LONG: "I", LONG8: "Q"}[typ], *values)

    def ifd(self, entries):
        """entries: [(tag, type, values)], written in tag order; returns the IFD's index."""
        inline = 8 if self.big else 4
        packed = []
        for tag, typ, values in sorted(entries, key=lambda t: t[0]):
            data = self.pack(typ, values)
            count = len(data) // _SIZE[typ]
            field = data.ljust(inline, b"\0") if len(data) <= inline else struct.pack(self.e + ("Q" if self.big else "I"), self.blob(data))
            packed.append((tag, typ, count, field))
        if len(self.buf) % 2:
            self.buf += b"\0"
        at = len(self.buf)
        index = len(self.ifd_at)
        self.ifd_at.append(at)
        struct.pack_into(self.e + ("Q" if self.big else "I"), self.buf, self.link, at)
        self.buf += struct.pack(self.e + ("Q" if self.big else "H"), len(packed))
        for tag, typ, count, field in packed:
            self.buf += struct.pack(self.e + ("HHQ" if self.big else "HHI"), tag, typ, count)
            self.count_at[(index, tag)] = len(self.buf) - (8 if self.big else 4)
            self.value_at[(index, tag)] = len(self.buf)
            self.buf += field
        self.link = len(self.buf)
        self.next_at.append(self.link)
        self.buf += struct.pack(self.e + ("Q" if self.big else "I"), 0)
        return index


def write_tiff(path, levels, *, tile=(256, 256), subsampling="4:2:0", tables=True, big=False, be=False, description=None,
               resolution=None, stripped_between=False, missing=(), progressive=(), other_sampling=(), truncated=(), compression=7,
               stripped_only=False):
    """Write ``levels`` (uint8 [h, w, 3] arrays, or [h, w] for ``subsampling="gray"``; widest first) as tiled IFDs.
    ``missing`` / ``progressive`` / ``other_sampling`` / ``truncated``: sets of (level, tx, ty) whose tile gets offset and count 0 /
    is coded progressively / at 4:4:4 instead / loses the second half of its stream.  ``resolution``: (x, y, unit).
    Returns a dict: ``streams[level][ty][tx]`` = the tile as a stand-alone JPEG stream, ``ifd_of_level``, and the writer's
    ``value_at`` / ``count_at`` / ``next_at`` / ``ifd_at`` offsets for tests that damage the file."""
    tw, th = tile
    w = _Writer(big, be)
    info = {"streams": [], "ifd_of_level": [], "tile": tile}
    off_type = LONG8 if big else LONG
    for li, px in enumerate(levels):
        if stripped_only or (stripped_between and li == 1):
            small = np.ascontiguousarray(levels[-1][:32, :48]) if levels[-1].ndim == 3 else np.zeros((32, 48, 3), np.uint8)
            strip = w.blob(small.tobytes())
            w.ifd([(256, LONG, [48]), (257, LONG, [32]), (258, SHORT, [8, 8, 8]), (259, SHORT, [1]), (262, SHORT, [2]),
                   (273, off_type, [strip]), (277, SHORT, [3]), (278, LONG, [32]), (279, off_type, [small.nbytes])])
            if stripped_only:
                break
        grey = px.ndim == 2
        h_img, w_img = px.shape[:2]
        nx, ny = -(-w_img // tw), -(-h_img // th)
        padded = np.empty((ny * th, nx * tw) + px.shape[2:], dtype=np.uint8)
        padded[...] = 255 if grey else PAD
        padded[:h_img, :w_img] = px
        offsets, counts, rows, jtables = [], [], [], None
        for ty in range(ny):
            row = []
            for tx in range(nx):
                key = (li, tx, ty)
                sub = "4:4:4" if key in other_sampling else subsampling
                full = encode_tile(padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw], sub, progressive=key in progressive)
                row.append(full)
                data = full
                if tables and key not in progressive and key not in other_sampling:
                    t, data = split_tables(full)
                    if jtables is None:
                        jtables = t
                    assert t == jtables, "tiles of one level share their tables"
                if key in truncated:
                    data = data[:len(data) // 2]
                if key in missing:
                    offsets.append(0)
                    counts.append(0)
                else:
                    offsets.append(w.blob(data))
                    counts.append(len(data))
            rows.append(row)
        entries = [(256, LONG, [w_img]), (257, LONG, [h_img]), (258, SHORT, [8] if grey else [8, 8, 8]), (259, SHORT, [compression]),
                   (262, SHORT, [1 if grey else 6]), (277, SHORT, [1 if grey else 3]), (284, SHORT, [1]),
                   (322, LONG, [tw]), (323, LONG, [th]), (324, off_type, offsets), (325, off_type, counts)]
        if not grey:
            entries.append((530, SHORT, list(_YCBCR_SUB[subsampling])))
        if tables and jtables is not None:
            entries.append((347, UNDEFINED, jtables))
        if description is not None and li == 0:
            entries.append((270, ASCII, description.encode("latin-1") + b"\0"))
        if resolution is not None:
            entries += [(282, RATIONAL, [(int(resolution[0] * 100), 100)]), (283, RATIONAL, [(int(resolution[1] * 100), 100)]),
                        (296, SHORT, [resolution[2]])]
        info["ifd_of_level"].append(w.ifd(entries))
        info["streams"].append(rows)
    with open(path, "wb") as fh:
        fh.write(bytes(w.buf))
    info.update(value_at=w.value_at, count_at=w.count_at, next_at=w.next_at, ifd_at=w.ifd_at, endian=w.e, big=big, size=len(w.buf))
    return info


def pillow_rgb(path, frame=0):
    """The oracle: Pillow (libtiff) reading the same file, uint8 [h, w, 3]."""
    with Image.open(path) as im:
        im.seek(frame)
        return np.asarray(im.convert("RGB"))


def assemble(info, level, width, height):
    """The same image from Pillow's decode of every tile as a stand-alone JPEG (equal to ``pillow_rgb`` wherever libtiff opens the
    file): the oracle for files libtiff refuses, such as one tile at another sampling than the YCbCrSubSampling tag states."""
    tw, th = info["tile"]
    rows = info["streams"][level]
    full = np.zeros((len(rows) * th, len(rows[0]) * tw, 3), dtype=np.uint8)
    for ty, row in enumerate(rows):
        for tx, stream in enumerate(row):
            with Image.open(io.BytesIO(stream)) as im:
                full[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = np.asarray(im.convert("RGB"))
    return full[:height, :width]


def crops(full, xy, w, h):
    """uint8 [n, h, w, 3]: crops of ``full`` at ``xy`` (x, y), zero-extended past the right and bottom (and left / top) edges."""
    out = np.zeros((len(xy), h, w, 3), dtype=np.uint8)
    H, W = full.shape[:2]
    for i, (x, y) in enumerate(xy):
        xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
        if xa < xb and ya < yb:
            out[i, ya - y:yb - y, xa - x:xb - x] = full[ya:yb, xa:xb]
    return out
