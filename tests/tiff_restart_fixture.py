"""Tiled-JPEG TIFF levels whose tiles carry restart intervals, generated at test time with ``tiff_fixture``'s writer.  No test of its own.

Every tile is a 4:2:0 stream written by Pillow with ``restart_marker_rows=1``.  Where the DRI segment stands is chosen per level:
  "tile"    in every tile's own (abbreviated) stream; the level's JPEGTables holds DQT / DHT only
  "both"    in every tile's own stream and once more in the level's JPEGTables stream, behind its DQT / DHT
  "tables"  in the level's JPEGTables stream alone.  libjpeg resets the interval at the tile's SOI and then warns about every marker: no
            reader takes such a level
The oracle is Pillow's decode of every tile as a stand-alone stream (``tiff_fixture.assemble``)."""
import io
import struct

import numpy as np
from PIL import Image

from tests import tiff_fixture as tf


def encode_tile(pixels, quality=80, **restart):
    buf = io.BytesIO()
    Image.fromarray(pixels, "RGB").save(buf, "JPEG", quality=quality, subsampling=2, **(restart or dict(restart_marker_rows=1)))
    return buf.getvalue()


def split_tables(stream, dri):
    """(tables-only stream, abbreviated stream): DQT / DHT moved out; the DRI segment copied ("both") or moved ("tables") with them."""
    assert stream[:2] == b"\xff\xd8"
    pos, tables, rest = 2, b"", b""
    while True:
        assert stream[pos] == 0xFF
        marker = stream[pos + 1]
        if marker == 0xDA:
            rest += stream[pos:]
            break
        length = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        seg = stream[pos:pos + 2 + length]
        if marker in (0xDB, 0xC4) or (marker == 0xDD and dri in ("both", "tables")):
            tables += seg
        if marker not in (0xDB, 0xC4) and not (marker == 0xDD and dri == "tables"):
            rest += seg
        pos += 2 + length
    return b"\xff\xd8" + tables + b"\xff\xd9", b"\xff\xd8" + rest


def write_tiff(path, levels, *, tile=(64, 64), dri=("tile", "both"), quality=80, damaged=None):
    """``levels``: uint8 [h, w, 3] arrays, widest first; ``dri[level]``: where the level's DRI segment stands.  ``damaged``: {(level, tx,
    ty): function stream -> stream} applied to the complete stream of a tile before it is stored (its tables are still split off).
    Returns ``streams[level][ty][tx]`` (the complete streams as stored, damage included), ``tables[level]`` and ``tile``."""
    tw, th = tile
    w = tf._Writer(False, False)
    info = {"streams": [], "tables": [], "tile": tile}
    for li, px in enumerate(levels):
        h_img, w_img = px.shape[:2]
        nx, ny = -(-w_img // tw), -(-h_img // th)
        padded = np.empty((ny * th, nx * tw, 3), dtype=np.uint8)
        padded[...] = tf.PAD
        padded[:h_img, :w_img] = px
        offsets, counts, rows, jtables = [], [], [], None
        for ty in range(ny):
            row = []
            for tx in range(nx):
                full = encode_tile(padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw], quality)
                if damaged and (li, tx, ty) in damaged:
                    full = damaged[(li, tx, ty)](full)
                row.append(full)
                t, data = split_tables(full, dri[li])
                jtables = t if jtables is None else jtables
                assert t == jtables, "tiles of one level share their tables"
                offsets.append(w.blob(data))
                counts.append(len(data))
            rows.append(row)
        assert (b"\xff\xdd" in jtables) == (dri[li] != "tile")
        w.ifd([(256, tf.LONG, [w_img]), (257, tf.LONG, [h_img]), (258, tf.SHORT, [8, 8, 8]), (259, tf.SHORT, [7]), (262, tf.SHORT, [6]),
               (277, tf.SHORT, [3]), (284, tf.SHORT, [1]), (322, tf.LONG, [tw]), (323, tf.LONG, [th]), (324, tf.LONG, offsets),
               (325, tf.LONG, counts), (530, tf.SHORT, [2, 2]), (347, tf.UNDEFINED, jtables)])
        info["streams"].append(rows)
        info["tables"].append(jtables)
    with open(path, "wb") as fh:
        fh.write(bytes(w.buf))
    return info
