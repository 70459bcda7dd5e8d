"""Launch trace of the SAM2 segmenter: every C-ABI call ``Sam2HipPredictor`` makes during one eager forward, as
``[name, arg, ...]`` with the arguments reduced to what decides the launch -- integers as they are, a ``c_float`` by its
float32 value, a float[3] by its values, a pointer as "null", "p16" (16-byte aligned) or "p" (``_lib.SIGNATURES`` tells
which is which).  tests/golden/sam2_launch_trace.json holds the recording the refactors of the predictor are held to:
``{mode: {batch size: [[count, name, arg, ...], ...]}}``, runs of identical consecutive calls collapsed into a count."""
import ctypes as C
import json
import os

from atlaspatch_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam2_launch_trace.json")
MODES = {"default": None, "exact_f32": "1"}          # mode -> ATLASPATCH_SAM2_EXACT_F32 before construction
BATCHES = (1, 2)
GEMM_ENTRIES = ("ap_gemm_split_f16", "ap_gemm_split_f16_windows", "ap_gemm", "ap_sgemm_stacked", "ap_sgemm")


def _log_arg(ctype, value):
    value = getattr(value, "value", value) if not isinstance(value, C.Array) else value
    if ctype is C.c_void_p:
        return "null" if not value else ("p16" if int(value) % 16 == 0 else "p")
    if ctype is C.c_float:
        return C.c_float(value).value
    if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
        return "null" if value is None else [C.c_float(v).value for v in value]
    return int(value)


class TracingLib:
    """Stands in for ``pred.lib``: forwards every call and logs it."""

    def __init__(self, lib):
        self._lib, self.records = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            assert len(args) == len(argtypes), name
            self.records.append([name] + [_log_arg(t, a) for t, a in zip(argtypes, args)])
            return fn(*args)
        return call


def collapse(records):
    out = []
    for r in records:
        if out and out[-1][1:] == r:
            out[-1][0] += 1
        else:
            out.append([1] + r)
    return out


def expand(collapsed):
    return [list(r[1:]) for r in collapsed for _ in range(r[0])]


def record_forward(pred, batch):
    """The calls of one eager ``_forward_masks`` on `batch` images (their content does not reach any argument)."""
    import torch
    imgs = torch.zeros((batch, 1024, 1024, 3), dtype=torch.uint8, device=pred.device)
    real, pred.lib = pred.lib, TracingLib(pred.lib)
    try:
        with torch.inference_mode(), torch.cuda.device(pred.device):
            pred._forward_masks(imgs)
            torch.cuda.synchronize(pred.device)
        return pred.lib.records
    finally:
        pred.lib = real


def record_mode(mode):
    """{batch size: collapsed trace} of a predictor on seeded random weights (seed 0) built in `mode`."""
    from atlaspatch_amd.services.sam2_hip import Sam2HipPredictor
    from atlaspatch_amd.services.segmentation import random_sam2_state_dict
    saved = os.environ.pop("ATLASPATCH_SAM2_EXACT_F32", None)
    try:
        if MODES[mode] is not None:
            os.environ["ATLASPATCH_SAM2_EXACT_F32"] = MODES[mode]
        pred = Sam2HipPredictor(random_sam2_state_dict(0), device="cuda")
    finally:
        os.environ.pop("ATLASPATCH_SAM2_EXACT_F32", None)
        if saved is not None:
            os.environ["ATLASPATCH_SAM2_EXACT_F32"] = saved
    try:
        return {str(b): collapse(record_forward(pred, b)) for b in BATCHES}
    finally:
        pred.close()


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def dump(trace, path):
    """One call per line: a diff of two recordings names the launches that moved."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (mode, per_batch) in enumerate(trace.items()):
            f.write(f' "{mode}": {{\n')
            for j, (b, rows) in enumerate(per_batch.items()):
                f.write(f'  "{b}": [\n' + ",\n".join("   " + json.dumps(r) for r in rows) + "\n  ]" + ("," if j + 1 < len(per_batch) else "") + "\n")
            f.write(" }" + ("," if i + 1 < len(trace) else "") + "\n")
        f.write("}\n")


def gemm_route_inputs(record, stack):
    """A GEMM record of the trace -> (entry point, keyword arguments of ``sam2_hip.gemm_route``).  `stack` is the number of
    images the row-wise layer ran on (the split-f16 and f32-wide entry points do not take it as an argument)."""
    name, a = record[0], record[1:]
    al = lambda p: p == "p16"
    if name == "ap_gemm_split_f16":
        _a, lda, _w, m, n, k, bias, act, resid, ldr, out, ldo = a[:12]
        kw = dict(stack=stack, act=act, lda=lda, ldw=k, ldo=ldo, ldr=ldr, w16=True)
    elif name == "ap_gemm_split_f16_windows":
        _a, lda, _w, m, n, k, bias, act, resid, ldr, out, ldo, _mode, stack = a[:14]
        kw = dict(stack=stack, act=act, lda=lda, ldw=k, ldo=ldo, ldr=ldr, w16=True, windows=True)
    elif name == "ap_gemm":
        _dt, act, _a, lda, _w, ldw, m, n, k, bias, resid, out, ldo = a[:13]
        kw = dict(stack=stack, act=act, lda=lda, ldw=ldw, ldo=ldo, ldr=n, w16=al(_w))
    elif name == "ap_sgemm_stacked":
        _a, lda, _w, ldw, stack, m, n, k, bias, act, resid, ldr, out, ldo = a[:14]
        kw = dict(stack=stack, act=act, lda=lda, ldw=ldw, ldo=ldo, ldr=ldr, w16=al(_w))
    elif name == "ap_sgemm":
        _a, lda, _sa, _w, ldw, _sw, w_kn, batch, m, n, k, alpha, bias, act, resid, ldr, _sr, out, ldo = a[:19]
        kw = dict(batch=batch, act=act, lda=lda, ldw=ldw, ldo=ldo, ldr=ldr, alpha=alpha, w_kn=bool(w_kn), w16=al(_w))
    else:
        raise KeyError(name)
    kw.update(rows=m // kw.get("stack", 1), n=n, k=k, bias=bias != "null", resid=resid != "null", a16=al(_a), out16=al(out),
              bias16=al(bias), resid16=al(resid))
    return name, kw
