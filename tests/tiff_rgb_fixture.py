"""RGB-coded JPEG tiles and tiled TIFF levels tagged PhotometricInterpretation 2, generated at test time with
``tiff_fixture``'s writer.  No test of its own.

Under tag 262 = 2 libtiff suppresses libjpeg's colour handling and hands a tile's three components out as R, G, B whatever the
stream's markers say.  Four kinds of tile stream stand under that tag here:
  "adobe"   Pillow ``keep_rgb=True, subsampling=0`` as written: Adobe marker with transform 0, component ids 'R' 'G' 'B'
  "ids123"  the same without its APPn segments and with the ids in SOF0 and SOS rewritten to 1 2 3 (libjpeg infers YCbCr)
  "ids012"  the same with ids 0 1 2 (libjpeg infers YCbCr)
  "ycc"     an ordinary YCbCr 4:4:4 stream from Pillow, unchanged: two quantisers, Huffman selectors 0/1/1; libtiff shows its
            Y, Cb, Cr planes as R, G, B
and "rgbids": "ids123" with ids 'R' 'G' 'B' (no marker: libjpeg infers RGB), for stand-alone files.
The oracle for a file is ``tiff_fixture.pillow_rgb`` (libtiff); for a stand-alone stream ``planes``: Pillow's decode with the
colour conversion switched off, which the CPU tests hold equal to libtiff's reading of the same stream under tag 262 = 2.
"""
import io
import struct

import numpy as np
from PIL import Image

from tests import jpeg_entropy_reference as eref
from tests import jpeg_reference as ref
from tests import tiff_fixture as tf

RGB = 4                                                 # AP_JPEG_RGB
KINDS = ("adobe", "ids123", "ids012", "ycc")
_IDS = {"ids123": bytes((1, 2, 3)), "ids012": bytes((0, 1, 2)), "rgbids": b"RGB"}


def image(width, height, seed=0):
    """``tiff_fixture.image`` with what drives the range limit: a 0 / 255 checkerboard per channel in the top-left 48 x 32 pixels of
    every 64 x 64 cell, and isolated extreme pixels."""
    out = tf.image(width, height, seed).copy()
    yy, xx = np.mgrid[0:height, 0:width]
    board = (yy % 64 < 32) & (xx % 64 < 48)
    for c in range(3):
        out[..., c][board] = ((((yy + xx + (c & 1)) & 1) * 255).astype(np.uint8))[board]
    out[5::23, 7::19] = (255, 0, 255)
    out[11::29, 3::17] = (0, 255, 0)
    return out


def relabel(stream, ids, keep_app=False):
    """The stream with the component ids of SOF0 and SOS rewritten to ``ids`` and (unless ``keep_app``) its APPn segments removed."""
    assert stream[:2] == b"\xff\xd8"
    out, pos = bytearray(b"\xff\xd8"), 2
    while True:
        assert stream[pos] == 0xFF
        marker = stream[pos + 1]
        length = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        seg = bytearray(stream[pos:pos + 2 + length])
        if marker == 0xC0:
            assert seg[9] == 3
            for c in range(3):
                seg[10 + 3 * c] = ids[c]
        if marker == 0xDA:
            assert seg[4] == 3
            for c in range(3):
                seg[5 + 2 * c] = ids[c]
            return bytes(out + seg + stream[pos + 2 + length:])
        if keep_app or not 0xE0 <= marker <= 0xEF:
            out += seg
        pos += 2 + length


def encode(pixels, kind, quality=80, **kw):
    """One tile of ``kind`` as a complete JPEG stream."""
    buf = io.BytesIO()
    if kind == "ycc":
        Image.fromarray(pixels, "RGB").save(buf, "JPEG", quality=quality, subsampling=0, **kw)
        return buf.getvalue()
    Image.fromarray(pixels, "RGB").save(buf, "JPEG", quality=quality, subsampling=0, keep_rgb=True, **kw)
    return buf.getvalue() if kind == "adobe" else relabel(buf.getvalue(), _IDS[kind])


def as_ycc(stream):
    """The same coefficients in a stream every reader takes for YCbCr 4:4:4: no APPn, ids 1 2 3.  Its slot under AP_JPEG_444 is what
    libjpeg's coefficient reader gives for ``stream``, whose colour model the slot does not record."""
    return relabel(stream, _IDS["ids123"])


def selectors(stream):
    """((dc, ac) per component) of the stream's scan header."""
    sos = stream.index(b"\xff\xda")
    return tuple((stream[sos + 6 + 2 * c] >> 4, stream[sos + 6 + 2 * c] & 15) for c in range(stream[sos + 4]))


def planes(stream):
    """uint8 [h, w, 3]: the three components as they are decoded, no colour conversion -- what libtiff shows under tag 262 = 2."""
    with Image.open(io.BytesIO(stream)) as im:
        if im.mode == "RGB" and stream.find(b"Adobe") < 0 and bytes(_sof_ids(stream)) != b"RGB":
            im.draft("YCbCr", im.size)                  # libjpeg infers YCbCr: ask for its planes, not for the conversion
            assert im.mode == "YCbCr"
        return np.asarray(im).copy()


def _sof_ids(stream):
    sof = stream.index(b"\xff\xc0")
    return [stream[sof + 10 + 3 * c] for c in range(stream[sof + 9])]


def sequential_slot(stream, side, tables=None):
    """(status, slot) of ``jpeg_entropy_reference``'s marker parser and sequential Huffman decode; the slot of an RGB-coded stream has
    the geometry of 4:4:4, so the stream is read as its YCbCr twin."""
    desc, payload = eref.parse(as_ycc(stream), side, ref.S444, tables)
    return eref.decode(desc, payload, side, ref.S444)


def staged_slot(raw_desc, arena, side):
    """(status, slot) decoded sequentially from a staged descriptor and its arena."""
    desc, payload = eref.unpack_descriptor(raw_desc, arena)
    return eref.decode(desc, payload, side, ref.S444)


def write_tiff(path, levels, *, tile=(48, 48), tables=True, big=False, be=False, missing=(), quality=80, photometric=2, progressive=False, description=None):
    """``levels``: [(uint8 [h, w, 3], kind)], widest first; kind one of KINDS (tag 262 = ``photometric``, no YCbCrSubSampling tag),
    "rgb420" (a 4:2:0 stream under tag 262 = 2, which libtiff rejects) or "ycbcr420" (an ordinary level: tag 262 = 6, 4:2:0).
    Edge tiles are stored full size, padded with ``tiff_fixture.PAD``.  ``missing``: (level, tx, ty) with offset and count 0.
    ``progressive``: the tiles of the KINDS levels are coded progressively (each with tables of its own: ``tables=False``).
    Returns ``streams[level][ty][tx]`` (complete streams) and ``tile``."""
    tw, th = tile
    w = tf._Writer(big, be)
    off_type = tf.LONG8 if big else tf.LONG
    info = {"streams": [], "tile": tile}
    for li, (px, kind) in enumerate(levels):
        h_img, w_img = px.shape[:2]
        nx, ny = -(-w_img // tw), -(-h_img // th)
        padded = np.empty((ny * th, nx * tw, 3), dtype=np.uint8)
        padded[...] = tf.PAD
        padded[:h_img, :w_img] = px
        offsets, counts, rows, jtables = [], [], [], None
        for ty in range(ny):
            row = []
            for tx in range(nx):
                cell = padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
                full = tf.encode_tile(cell, "4:2:0", quality=quality) if kind in ("rgb420", "ycbcr420") else encode(cell, kind, quality, progressive=progressive)
                row.append(full)
                data = full
                if tables:
                    t, data = tf.split_tables(full)
                    jtables = t if jtables is None else jtables
                    assert t == jtables, "tiles of one level share their tables"
                if (li, tx, ty) in missing:
                    offsets.append(0)
                    counts.append(0)
                else:
                    offsets.append(w.blob(data))
                    counts.append(len(data))
            rows.append(row)
        entries = [(256, tf.LONG, [w_img]), (257, tf.LONG, [h_img]), (258, tf.SHORT, [8, 8, 8]), (259, tf.SHORT, [7]),
                   (262, tf.SHORT, [6 if kind == "ycbcr420" else photometric]), (277, tf.SHORT, [3]), (284, tf.SHORT, [1]),
                   (322, tf.LONG, [tw]), (323, tf.LONG, [th]), (324, off_type, offsets), (325, off_type, counts)]
        if kind == "ycbcr420":
            entries.append((530, tf.SHORT, [2, 2]))
        if tables and jtables is not None:
            entries.append((347, tf.UNDEFINED, jtables))
        if description is not None and li == 0:
            entries.append((270, tf.ASCII, description.encode("latin-1") + b"\0"))
        w.ifd(entries)
        info["streams"].append(rows)
    with open(path, "wb") as fh:
        fh.write(bytes(w.buf))
    return info


def tiles_of(full, tile, nx, ny):
    """uint8 [ny * nx, th, tw, 3]: the tiles of a level image in tile-id order, the part past the image's edge zero."""
    tw, th = tile
    return tf.crops(full, [(tx * tw, ty * th) for ty in range(ny) for tx in range(nx)], tw, th)


def open_tiff(path):
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    wsi = TiffWSI(str(path))
    wsi._ensure_loaded()
    return wsi


def tiff_slots(lib, wsi, level, ids, poison=0xA5):
    """(return code, uint8 [m, slot_bytes]) of ap_host_tiff_tile_coefficients on poisoned slots of the level's own sampling."""
    lv = wsi.levels[level]
    stride = lib.ap_jpeg_slot_bytes_ex(lv["tw"], max(lv["sampling"], 0))
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    slots = np.full((ids.shape[0], stride), poison, dtype=np.uint8)
    return lib.ap_host_tiff_tile_coefficients(wsi._handle, level, ids.ctypes.data, ids.shape[0], slots.ctypes.data), slots


def tiff_streams(lib, wsi, level, ids, poison=0xA5):
    """(return code, descs uint8 [m, 2048], arena, used) of ap_host_tiff_tile_streams on poisoned, 16-byte aligned buffers."""
    import ctypes as C
    from tests import jpeg_entropy_streams as es
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    m = ids.shape[0]
    bound = lib.ap_host_tiff_max_tile_bytes(wsi._handle, level)
    descs = es._aligned(m * eref.HEADER_BYTES, poison).reshape(m, eref.HEADER_BYTES)
    arena = es._aligned(max(m * bound, 16), poison)
    used = C.c_size_t()
    rc = lib.ap_host_tiff_tile_streams(wsi._handle, level, ids.ctypes.data, m, descs.ctypes.data, arena.ctypes.data, arena.shape[0], C.byref(used))
    return rc, descs, arena, used.value


def rgb_store(folder, full, quality=80):
    """A JPEG ``.synth`` store of the 256-px tiles of ``full`` on the tile grid, every tile of kind "adobe" (what libjpeg itself infers
    as RGB): (slide path, coords int32 [n, 5], uint8 [n, 256, 256, 3] = Pillow's decode of every stored tile)."""
    import json
    height, width = full.shape[:2]
    store = folder / "tiles"
    store.mkdir(parents=True)
    slide = folder / "j.synth"
    slide.write_text(json.dumps({"width": width, "height": height, "seed": 7, "n_ellipses": 3, "mag": 20, "mpp": 0.5,
                                 "downsamples": [1, 4, 16], "jpeg_tiles": "tiles"}))
    coords = np.array([[x, y, 256, 256, 0] for y in range(0, height, 256) for x in range(0, width, 256)], dtype=np.int32)
    tiles = []
    for x, y in coords[:, :2].tolist():
        path = store / f"{x}_{y}_256.jpg"
        path.write_bytes(encode(np.ascontiguousarray(full[y:y + 256, x:x + 256]), "adobe", quality))
        with Image.open(path) as im:
            tiles.append(np.asarray(im.convert("RGB")))
    return str(slide), coords, np.stack(tiles)
