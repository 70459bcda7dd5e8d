"""The checkers the far-offset tests share (tests/test_gpu_far_rows.py, tests/test_gpu_far_tiles.py): poisoned regions between
guard bands, seeded fillers that can make any rows again, the chunk walker, and -- for operators that map image i of their
operands to image i of their output -- the three checks A (every image equals the same image computed alone, bit for bit),
B (sampled images against a reference) and C (stray and missing writes).  A helper, not a test.

Nothing here needs a GPU: every class takes the device it works on, and the sizes that are tied to the lines (the elements
one torch call touches, the scratch of a chunk, the guard bands) scale with a ``line`` parameter.  ``line`` is the byte offset
that plays the part of 2^31: with line = 2^16 the same code runs on CPU tensors of a few hundred KiB, where
tests/test_far_tiles_cpu.py drives it with operators whose offsets wrap at the line."""
import torch

from tests import far_rows as F
from tests.helpers import PATTERN

LINE = 1 << 31                   # the byte offset the lines are multiples of: 2^31 on the device
STEP = 1 << 27                   # elements per torch call on a large buffer
SCRATCH = 1 << 30                # bytes of a chunk's scratch operand
GUARD = 1 << 14                  # elements of a guard band (a multiple of 128: the payload keeps the allocation's alignment)
POISON = {1: 0xFF, **PATTERN}    # per element size: a byte the u8 cases cannot produce, the NaN patterns of tests/helpers.py


def scaled(value, line):
    """A size tied to the lines (STEP, SCRATCH, GUARD) at another line; never below 64."""
    return value if line == LINE else max(64, value // (LINE // line))


def limit_of(name, line=LINE):
    """(offset, unit) of a key of far_rows.LINES with `line` in the place of 2^31."""
    limit, unit = F.LINES[name]
    return limit // (LINE // line), unit


def straddling_row(width, es, name, line=LINE):
    """far_rows.straddling_row with `line` in the place of 2^31."""
    if line == LINE:
        return F.straddling_row(width, es, name)
    limit, unit = limit_of(name, line)
    return (limit if unit == "elements" else -(-limit // es)) // width


def crossings(rows, width, es, line=LINE):
    """{line name: straddling row} for the lines a dense [rows, width] buffer reaches."""
    return {name: straddling_row(width, es, name, line) for name in F.LINES if straddling_row(width, es, name, line) < rows}


def sample_images(n, buffers, line=LINE, live=None):
    """Sorted image indices: the first, the image that owns the element at each line of every buffer (per, es) -- elements per
    image, element size --, the last of `live` (n by default)."""
    live = n if live is None else live
    pick = {0, live - 1}
    for per, es in buffers:
        pick |= {F.image_of(r, 1) for r in crossings(n, per, es, line).values() if r < live}
    return sorted(pick)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _poison(t, step=STEP):
    """The poison pattern into a contiguous tensor of any size, `step` elements per call."""
    flat = t.view(-1)
    for o in range(0, flat.numel(), step):
        _bits(flat[o:o + step]).fill_(POISON[t.element_size()])
    return t


def _pattern_count(t, step=STEP):
    flat, n = t.view(-1), 0
    for o in range(0, flat.numel(), step):
        n += int((_bits(flat[o:o + step]) == POISON[t.element_size()]).sum())
    return n


def _same(x, y):
    """x and y (contiguous, below 2^31 elements) hold the same bits."""
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))


class Region:
    """Consecutive dense [rows, width] segments of one type between two guard bands, everything filled with the poison pattern."""

    def __init__(self, dev, dtype, *shapes, line=LINE):
        self.guard, self.step = scaled(GUARD, line), scaled(STEP, line)
        numel = sum(r * w for r, w in shapes)
        self.flat = _poison(torch.empty(numel + 2 * self.guard, dtype=dtype, device=dev), self.step)
        self.parts, off = [], self.guard
        for r, w in shapes:
            self.parts.append(self.flat[off:off + r * w].view(r, w))
            off += r * w
        self.t = self.parts[0]
        assert self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        want = POISON[self.flat.element_size()]
        return bool((_bits(self.flat[:self.guard]) == want).all()) and bool((_bits(self.flat[-self.guard:]) == want).all())


class Filler:
    """Seeded normal values for a [rows, width] buffer, made on the device in chunks of `step` rows; any rows can be made again."""

    def __init__(self, dev, dtype, rows, width, seed, scale=1.0, shift=0.0):
        self.dev, self.dtype, self.total, self.width, self.seed, self.scale, self.shift = dev, dtype, rows, width, seed, scale, shift
        self.step = max(256, STEP // width // 256 * 256)

    def chunk(self, ci):
        n = min(self.step, self.total - ci * self.step)
        g = torch.Generator(device=self.dev).manual_seed(self.seed * 1000003 + ci)
        x = torch.randn(n, self.width, generator=g, device=self.dev, dtype=torch.float32)
        return (x * self.scale + self.shift).to(self.dtype)

    def chunks(self):
        for ci in range(-(-self.total // self.step)):
            yield ci * self.step, min(self.total, (ci + 1) * self.step), ci

    def fill(self, t):
        for r0, r1, ci in self.chunks():
            t[r0:r1].copy_(self.chunk(ci))

    def unchanged(self, t):
        return all(_same(t[r0:r1], self.chunk(ci)) for r0, r1, ci in self.chunks())

    def rows(self, r0, r1):
        parts = [self.chunk(ci)[max(r0, c0) - c0:min(r1, c1) - c0] for c0, c1, ci in self.chunks() if c0 < r1 and r0 < c1]
        return torch.cat(parts) if len(parts) > 1 else parts[0].clone()


class ImageFiller(Filler):
    """A Filler for [images, elements per image]: chunks of whole images, uint8 values uniform in [lo, hi] or, for the other
    types, scaled and shifted normal values; or whatever `make(generator, first image, images)` returns."""

    def __init__(self, dev, dtype, images, per, seed, lo=0, hi=255, scale=1.0, shift=0.0, make=None, line=LINE):
        super().__init__(dev, dtype, images, per, seed, scale, shift)
        self.step = max(1, scaled(STEP, line) // per)
        self.lo, self.hi, self.make = lo, hi, make

    def chunk(self, ci):
        n = min(self.step, self.total - ci * self.step)
        g = torch.Generator(device=self.dev).manual_seed(self.seed * 1000003 + ci)
        if self.make is not None:
            return self.make(g, ci * self.step, n)
        if self.dtype in (torch.uint8, torch.int32):
            return torch.randint(self.lo, self.hi + 1, (n, self.width), generator=g, device=self.dev, dtype=self.dtype)
        return super().chunk(ci)


def _walk(rows, unit_rows, row_bytes, line=LINE):
    """(r0, r1) chunks of whole units (256 rows, an image) whose widest operand stays within the scratch (2^30 bytes at the
    device's line)."""
    per = max(1, scaled(SCRATCH, line) // (row_bytes * unit_rows)) * unit_rows
    return [(r0, min(rows, r0 + per)) for r0 in range(0, rows, per)]


# ----------------------------------------------------------------------------- operators that map image i to image i
class ImageOp:
    """What FarRun needs of an operator.  ``ins``: ((name, elements per image, dtype, filler arguments), ...), ``outs``: ((name,
    elements per image, dtype), ...).  ``launch(n, ins, outs)`` runs the operator on the first n images of the given tensors
    ([images, elements]); ``reference(i, ins, gots)`` judges image i from CPU copies of its operands and its outputs and returns
    None or a description of the failure.  ``clean`` is False where an output can hold the poison value by right (check C
    then leaves the count of poisoned elements out)."""
    id, ins, outs, clean = "", (), (), True

    def launch(self, n, ins, outs):
        raise NotImplementedError

    def reference(self, i, ins, gots):
        raise NotImplementedError

    def alone(self, run, i0, i1, outs):
        """Images i0 .. i1 of the far problem computed alone, from copies of their operands, into `outs`."""
        self.launch(i1 - i0, [r.t[i0:i1].clone() for r in run.ins], outs)


class FarRun:
    """One operator on n images in regions of their own; the checks A, B and C of the module docstring."""

    def __init__(self, op, n, dev, line=LINE):
        self.op, self.n, self.dev, self.line = op, n, dev, line
        self.step = scaled(STEP, line)
        self.ins, self.fillers = [], []
        for k, (_, per, dtype, kw) in enumerate(op.ins):
            self.ins.append(Region(dev, dtype, (n, per), line=line))
            self.fillers.append(ImageFiller(dev, dtype, n, per, seed=17 + k, line=line, **kw))
            self.fillers[-1].fill(self.ins[-1].t)
        self.outs = [Region(dev, dtype, (n, per), line=line) for _, per, dtype in op.outs]

    def buffers(self):
        """(elements per image, element size) of every region: what the sampled images are chosen by."""
        return [(r.t.shape[1], r.t.element_size()) for r in self.ins + self.outs]

    def names(self):
        return [spec[0] for spec in tuple(self.op.ins) + tuple(self.op.outs)]

    def far(self, live=None):
        """The far launch on the first `live` images, every output poisoned first."""
        for r in self.outs:
            _poison(r.t, self.step)
        self.op.launch(self.n if live is None else live, [r.t for r in self.ins], [r.t for r in self.outs])

    def check_c(self, live=None):
        live, c = self.n if live is None else live, self.op.id
        for r, name in zip(self.ins + self.outs, self.names()):
            assert r.guards_intact(), f"{c}: C: a guard band of {name} was written"
        for r, (name, per, _) in zip(self.outs, self.op.outs):
            left = _pattern_count(r.t[:live], self.step) if self.op.clean else 0
            assert left == 0, f"{c}: C: {left} elements of {name} were not written"
            assert _pattern_count(r.t[live:], self.step) == (self.n - live) * per, f"{c}: C: {name} was written behind the last image"
        for r, f, name in zip(self.ins, self.fillers, self.names()):
            assert f.unchanged(r.t), f"{c}: C: {name} was written"

    def check_a(self):
        walk = _walk(self.n, 1, max(per * es for per, es in self.buffers()), self.line)
        scratch = [torch.empty((walk[0][1], r.t.shape[1]), dtype=r.t.dtype, device=self.dev) for r in self.outs]
        for i0, i1 in walk:
            so = [_poison(s[:i1 - i0], self.step) for s in scratch]
            self.op.alone(self, i0, i1, so)
            for s, r, (name, *_) in zip(so, self.outs, self.op.outs):
                assert _same(s, r.t[i0:i1]), f"{self.op.id}: A: images {i0} .. {i1 - 1} of {name} differ from the same images computed alone"
        return len(walk)

    def check_b(self, images):
        failed = []
        for i in images:
            bad = self.op.reference(i, [r.t[i].cpu() for r in self.ins], [r.t[i].cpu() for r in self.outs])
            if bad is not None:
                failed.append((i, bad))
        assert not failed, f"{self.op.id}: B: images that miss the reference {failed}"

    def all_checks(self):
        """The whole far problem under C, A and B, then the ragged launch (one image fewer on the same buffers) under C and B.
        Returns (chunks walked, images sampled)."""
        self.far()
        self.check_c()
        chunks = self.check_a()
        images = sample_images(self.n, self.buffers(), self.line)
        self.check_b(images)
        self.far(self.n - 1)
        self.check_c(self.n - 1)
        self.check_b([self.n - 2] if self.n > 1 else [])
        return chunks, images
