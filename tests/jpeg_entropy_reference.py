"""Plain sequential restatement of the stream route's two halves, the readable statement of what ``ap_host_jpeg_streams`` stages and
``ap_jpeg_entropy_decode_tiles`` must produce: marker parse -> descriptor + unstuffed payload -> Huffman decode -> coefficient slot.
Holds no test of its own; tests/test_jpeg_entropy_cpu.py pins it against libjpeg (``ap_host_jpeg_coefficients``).

Descriptor (csrc/jpeg_stream.h), 2048 bytes: uint16 quant[3][64] natural order | uint8 counts[4][16] (DC0, DC1, AC0, AC1) |
uint8 symbols[4][256] | dc_sel[3], 0 | ac_sel[3], 0 | uint32 ncomp | uint32 payload_bytes | uint64 payload_offset | zeros."""
import struct

import numpy as np

from tests import jpeg_reference as ref

HEADER_BYTES = 2048
OK, BAD_CODE, BAD_INDEX, EXHAUSTED, LEFTOVER, BAD_DESCRIPTOR = 0, 1, 2, 3, 4, 5
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


class Refused(ValueError):
    pass


def _segments(data, at):
    """(marker, body) from byte ``at`` up to and including SOS; then the offset behind the SOS header."""
    out = []
    while True:
        if at >= len(data) or data[at] != 0xFF:
            raise Refused("stream cut inside a header")
        while at < len(data) and data[at] == 0xFF:
            at += 1
        if at >= len(data):
            raise Refused("stream cut inside a header")
        m = data[at]
        at += 1
        if m in (0xD8, 0x01):
            continue
        if m == 0xD9:
            out.append((m, b""))
            return out, at
        if 0xD0 <= m <= 0xD7:
            raise Refused("restart marker outside a scan")
        if len(data) - at < 2:
            raise Refused("stream cut inside a header")
        length = (data[at] << 8) | data[at + 1]
        if length < 2 or length > len(data) - at:
            raise Refused("segment length runs past the buffer")
        out.append((m, bytes(data[at + 2:at + length])))
        at += length
        if m == 0xDA:
            return out, at


def _tables_from(segments, t):
    for m, body in segments:
        if m == 0xDB:
            while body:
                pq, tq = body[0] >> 4, body[0] & 15
                need = 1 + (128 if pq else 64)
                if pq > 1 or tq > 3 or len(body) < need:
                    raise Refused("DQT")
                vals = struct.unpack(">64H", body[1:need]) if pq else body[1:need]
                q = [0] * 64
                for k in range(64):
                    q[ZIGZAG[k]] = vals[k]
                t["quant"][tq] = q
                body = body[need:]
        elif m == 0xC4:
            while body:
                if len(body) < 17:
                    raise Refused("DHT")
                tc, th = body[0] >> 4, body[0] & 15
                counts = list(body[1:17])
                total = sum(counts)
                if tc > 1 or th > 1 or total > 256 or len(body) < 17 + total:
                    raise Refused("DHT")
                code, last = 0, max([l + 1 for l in range(16) if counts[l]], default=0)
                for l in range(1, last + 1):
                    code += counts[l - 1]
                    if code >= 1 << l:
                        raise Refused("over-subscribed code")
                    code <<= 1
                symbols = list(body[17:17 + total])
                if tc == 0 and any(s > 15 for s in symbols):
                    raise Refused("DC category")
                t["huff"][2 * tc + th] = (counts, symbols)
                body = body[17 + total:]
        elif m == 0xE0 and len(body) >= 14 and body[:5] == b"JFIF\0":
            t["jfif"] = True
        elif m == 0xEE and len(body) >= 12 and body[:5] == b"Adobe":
            t["adobe"] = body[11]
        elif m == 0xDD:
            t["restart"] = (body[0] << 8) | body[1]


def parse(stream, side, sampling, tables=None):
    """-> (descriptor dict, payload bytes), or raises ``Refused`` with the reason."""
    t = {"quant": {}, "huff": {}, "jfif": False, "adobe": None, "restart": 0}
    if tables:
        if tables[:2] != b"\xff\xd8":
            raise Refused("JPEGTables")
        _tables_from(_segments(tables, 2)[0], t)
    if stream[:2] != b"\xff\xd8":
        raise Refused("not a JPEG stream")
    segments, at = _segments(stream, 2)
    _tables_from(segments, t)
    frame = None
    for m, body in segments:
        if m in (0xC2, 0xC6, 0xCA, 0xCE):
            raise Refused("progressive stream")
        if m in (0xC9, 0xCB, 0xCC, 0xCD, 0xCF):
            raise Refused("arithmetic-coded stream")
        if m in (0xC1, 0xC3, 0xC5, 0xC7):
            raise Refused("not baseline")
        if m == 0xC0:
            if body[0] != 8 or body[5] not in (1, 3) or len(body) != 6 + 3 * body[5]:
                raise Refused("SOF0")
            frame = dict(height=(body[1] << 8) | body[2], width=(body[3] << 8) | body[4],
                         comps=[(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])])
    m, sos = segments[-1]
    if m != 0xDA or frame is None:
        raise Refused("no scan")
    comps = frame["comps"]
    if sos[0] != len(comps) or len(sos) != 4 + 2 * sos[0] or tuple(sos[-3:]) != (0, 63, 0):
        raise Refused("the scan does not hold all components")
    sel = []
    for c, (cid, _, _, _) in enumerate(comps):
        if sos[1 + 2 * c] != cid:
            raise Refused("components out of order")
        dc, ac = sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15
        if dc > 1 or ac > 1 or dc not in t["huff"] or 2 + ac not in t["huff"]:
            raise Refused("a Huffman table that does not exist")
        sel.append((dc, ac))
    hv = [(h, v) for _, h, v, _ in comps]
    if len(comps) == 1:
        found = ref.GRAY if hv[0] == (1, 1) else -1
    else:
        rgb = False if t["jfif"] else t["adobe"] == 0 if t["adobe"] is not None else bytes(c[0] for c in comps) == b"RGB"
        if rgb:
            raise Refused("RGB")
        found = {(1, 1): ref.S444, (2, 1): ref.S422, (2, 2): ref.S420}.get(hv[0], -1) if hv[1:] == [(1, 1), (1, 1)] else -1
    if found < 0 or found != sampling:
        raise Refused("sampling")
    if (frame["width"], frame["height"]) != (side, side):
        raise Refused("tile size")
    hmax, vmax = (2 if sampling >= ref.S422 else 1), (2 if sampling == ref.S420 else 1)
    if side > 976 or side % (8 * hmax) or side % (8 * vmax):
        raise Refused("side is no multiple of the MCU size")
    if t["restart"]:
        raise Refused("restart interval")
    if any(c[3] not in t["quant"] for c in comps):
        raise Refused("a quantisation table that does not exist")
    payload, i = bytearray(), at
    while i < len(stream):
        b = stream[i]
        if b != 0xFF:
            payload.append(b)
            i += 1
            continue
        if i + 1 >= len(stream):
            break
        nx = stream[i + 1]
        if nx == 0:
            payload.append(0xFF)
            i += 2
        elif nx == 0xFF:
            i += 1
        elif 0xD0 <= nx <= 0xD7:
            raise Refused("restart marker in the scan")
        else:
            break
    desc = dict(quant=[t["quant"][c[3]] for c in comps], huff=[t["huff"].get(s, ([0] * 16, [])) for s in range(4)], sel=sel,
                ncomp=len(comps))
    return desc, bytes(payload)


def pack_descriptor(desc, payload_offset, payload_bytes):
    """The descriptor as the 2048 bytes the host stager writes."""
    out = bytearray(HEADER_BYTES)
    for c, q in enumerate(desc["quant"]):
        out[128 * c:128 * c + 128] = struct.pack("<64H", *q)
    for s, (counts, symbols) in enumerate(desc["huff"]):
        out[384 + 16 * s:384 + 16 * s + 16] = bytes(counts)
        out[448 + 256 * s:448 + 256 * s + len(symbols)] = bytes(symbols)
    for c, (dc, ac) in enumerate(desc["sel"]):
        out[1472 + c], out[1476 + c] = dc, ac
    out[1480:1496] = struct.pack("<IIQ", desc["ncomp"], payload_bytes, payload_offset)
    return bytes(out)


def unpack_descriptor(raw, arena):
    """(descriptor dict, payload bytes) from a staged descriptor and its arena."""
    raw = bytes(raw)
    ncomp, nbytes, offset = struct.unpack("<IIQ", raw[1480:1496])
    huff = []
    for s in range(4):
        counts = list(raw[384 + 16 * s:384 + 16 * s + 16])
        huff.append((counts, list(raw[448 + 256 * s:448 + 256 * s + min(256, sum(counts))])))
    desc = dict(quant=[list(struct.unpack("<64H", raw[128 * c:128 * c + 128])) for c in range(ncomp)], huff=huff,
                sel=[(raw[1472 + c], raw[1476 + c]) for c in range(ncomp)], ncomp=ncomp)
    return desc, bytes(arena[offset:offset + nbytes])


_LOOKUP = {}


def _lookup(counts, symbols):
    """16-bit look-ahead: entry = (length << 8) | symbol, 0 where no code matches."""
    key = (tuple(counts), tuple(symbols))
    if key not in _LOOKUP:
        table = np.zeros(65536, dtype=np.int32)
        code, p = 0, 0
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                lo = code << (16 - l)
                table[lo:lo + (1 << (16 - l))] = (l << 8) | symbols[p]
                code += 1
                p += 1
            code <<= 1
        _LOOKUP[key] = table.tolist()
    return _LOOKUP[key]


def decode(desc, payload, side, sampling, stats=None):
    """-> (status, slot uint8 [slot_bytes]).  Sequential: MCU by MCU, block by block, symbol by symbol.  ``stats`` (a dict) collects
    what the corpus test asserts: the longest code used, ZRL symbols, blocks that end on coefficient 63 without an EOB."""
    comps, nbytes = ref.geometry(side, sampling)
    slot = np.zeros(nbytes, dtype=np.uint8)
    for c, q in enumerate(desc["quant"]):
        slot[128 * c:128 * c + 128] = np.frombuffer(struct.pack("<64H", *q), dtype=np.uint8)
    coef = slot[ref.HEADER:].view(np.int16)
    hmax, vmax = (2 if sampling >= ref.S422 else 1), (2 if sampling == ref.S420 else 1)
    mcux, mcuy = side // (8 * hmax), side // (8 * vmax)
    dc_tab = [_lookup(*desc["huff"][dc]) for dc, _ in desc["sel"]]
    ac_tab = [_lookup(*desc["huff"][2 + ac]) for _, ac in desc["sel"]]
    blocks = [(0, dy, dx) for dy in range(vmax) for dx in range(hmax)] + [(c, 0, 0) for c in range(1, len(comps))]
    buf, nbits, p = payload + b"\0\0\0\0", 8 * len(payload), 0
    last_dc = [0] * len(comps)
    longest = zrl = full = 0
    for my in range(mcuy):
        for mx in range(mcux):
            for c, dy, dx in blocks:
                _, _, wb, _, off = comps[c]
                h, v = (hmax, vmax) if c == 0 else (1, 1)
                base = (off - ref.HEADER) // 2 + ((my * v + dy) * wb + mx * h + dx) * 64
                z = 0
                while True:
                    word = (int.from_bytes(buf[p >> 3:(p >> 3) + 4], "big") << (p & 7)) & 0xFFFFFFFF
                    entry = (dc_tab[c] if z == 0 else ac_tab[c])[word >> 16]
                    if entry == 0:
                        return BAD_CODE, slot
                    l, sym = entry >> 8, entry & 255
                    longest = max(longest, l)
                    p += l
                    run, s = (0, sym & 15) if z == 0 else (sym >> 4, sym & 15)
                    if z and s == 0:
                        if run != 15:
                            if p > nbits:
                                return EXHAUSTED, slot
                            break
                        zrl += 1
                        z += 16
                        if z > 63:
                            return BAD_INDEX, slot
                        if p > nbits:
                            return EXHAUSTED, slot
                        continue
                    z += run
                    if z > 63:
                        return BAD_INDEX, slot
                    x = 0
                    if s:
                        word = (int.from_bytes(buf[p >> 3:(p >> 3) + 4], "big") << (p & 7)) & 0xFFFFFFFF
                        x = word >> (32 - s)
                        if x < 1 << (s - 1):
                            x -= (1 << s) - 1
                        p += s
                    if p > nbits:
                        return EXHAUSTED, slot
                    if z == 0:
                        last_dc[c] += x
                        x = last_dc[c]
                    coef[base + ZIGZAG[z]] = ((x + 32768) & 0xFFFF) - 32768          # int16 by C truncation
                    z += 1
                    if z == 64:
                        full += 1
                        break
    if stats is not None:
        stats["longest"] = max(stats.get("longest", 0), longest)
        stats["zrl"] = stats.get("zrl", 0) + zrl
        stats["full"] = stats.get("full", 0) + full
    if nbits - p >= 8:
        return LEFTOVER, slot
    return OK, slot


def outside_padding(slot):
    """The bytes of a slot (or of rows of slots) that are specified: 0 .. 383 and 512 onwards."""
    slot = np.asarray(slot)
    return np.concatenate([slot[..., :384], slot[..., 512:]], axis=-1)
