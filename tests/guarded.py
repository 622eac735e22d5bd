"""Guard bands round every device buffer the Python layer hands to the library.

Every call buffer of mocodad_amd/engine.py and mocodad_amd/stream.py comes from torch.empty / empty_like / zeros / full.  Inside
`guarded()` the name `torch` of those two modules is a GuardedTorch: it forwards everything else, and carves each device result
of those four out of a uint8 backing tensor laid out as

    [ guard | interior | guard ]      guard = max(GUARD, bytes of one leading-index row) rounded up to 256, bytes GUARD_BYTE

The interior of empty / empty_like is POISON (0xFF: float32 / float64 NaN with all bits set, int -1 -- a pattern the library
never produces, its own NaN is 0x7fc00000); the interior of zeros / full holds what was asked for.  The proxy keeps every
backing tensor, so no block is recycled before check() has looked at it:

    with guarded() as g:
        sc._ws.clear()                      # a cached workspace would not be a guarded one
        loss, poses = sc.score(...)
        torch.cuda.synchronize()
        g.check()                           # every guard byte is still GUARD_BYTE, else GuardViolation naming the allocation
        assert unwritten(loss) == 0         # no element still holds POISON

guarded_copy(t, fill) puts an input the test owns between bands of all-ones NaNs or of finite random floats: a result that
depends on memory outside its inputs differs between the two.  A plain helper module: no fixture, no pytest setting."""
import contextlib
import os
import sys

import torch as _torch

GUARD = 4096
GUARD_BYTE = 0xA5
POISON = 0xFF
_WRAPPED = ("empty", "empty_like", "zeros", "full")


class GuardViolation(AssertionError):
    pass


def _round256(n):
    return (int(n) + 255) // 256 * 256


def _guard_bytes(shape, itemsize):
    row = itemsize
    for d in shape[1:]:
        row *= int(d)
    return max(GUARD, _round256(row)), row


class GuardedTorch:
    """Stands in for the module `torch`.  guard_cpu: CPU results are carved too (the host tests; on the device path a CPU or
    pinned result passes through).  short_rows: the interior is that many leading-index rows shorter than the tensor handed out,
    whose last rows then lie in the tail guard, inside the backing tensor (the sensitivity test)."""

    def __init__(self, guard_cpu=False, short_rows=0):
        self._real = _torch
        self._guard_cpu = bool(guard_cpu)
        self._short_rows = int(short_rows)
        self.registry = []

    def __getattr__(self, name):
        return getattr(self._real, name)

    # ---- the four allocating functions (the shape and dtype rules are torch's own: asked of a meta tensor)
    @staticmethod
    def _meta(kw):
        return {**{k: v for k, v in kw.items() if k not in ("pin_memory", "out")}, "device": "meta"}

    def empty(self, *size, **kw):
        return self._alloc("empty", self._real.empty(*size, **self._meta(kw)), kw, None)

    def zeros(self, *size, **kw):
        return self._alloc("zeros", self._real.empty(*size, **self._meta(kw)), kw, 0)

    def full(self, size, fill_value, **kw):
        return self._alloc("full", self._real.full(size, fill_value, **self._meta(kw)), kw, fill_value)

    def empty_like(self, t, **kw):
        if not t.is_contiguous():
            raise NotImplementedError("GuardedTorch.empty_like: only contiguous tensors (what engine.py and stream.py pass)")
        kw.setdefault("device", t.device)
        return self._alloc("empty_like", self._real.empty(t.shape, dtype=kw.get("dtype", t.dtype), device="meta"), kw, None)

    def _alloc(self, fn, meta, kw, fill):
        dev = self._real.device(kw["device"]) if kw.get("device") is not None else self._real.device("cpu")
        shape, dtype = tuple(meta.shape), meta.dtype
        on_device = dev.type == "cuda" or (self._guard_cpu and not kw.get("pin_memory"))
        if not on_device or meta.numel() == 0 or kw.get("out") is not None:
            real = getattr(self._real, fn)
            return real(shape, fill, **kw) if fn == "full" else real(shape, **kw)
        itemsize = meta.element_size()
        nbytes = meta.numel() * itemsize
        guard, row = _guard_bytes(shape, itemsize)
        interior = nbytes - self._short_rows * row
        if interior < 0:
            raise ValueError(f"short_rows {self._short_rows}: the tensor {shape} has fewer rows")
        backing = self._real.full((guard + interior + guard,), GUARD_BYTE, dtype=self._real.uint8, device=dev)
        t = backing[guard:guard + nbytes].view(dtype).view(shape)
        if fill is None:
            backing[guard:guard + interior] = POISON
        elif interior == nbytes:
            t.fill_(fill)
        else:
            backing[guard:guard + interior] = 0
        self.registry.append({"backing": backing, "guard": guard, "nbytes": interior, "shape": shape, "dtype": dtype, "fn": fn,
                              "where": _caller()})
        return t

    # ---- the checks
    def allocations(self):
        """-> ['engine.py:298 _score: empty (3, 2) float32', ...] in allocation order"""
        return [_name(e) for e in self.registry]

    def violations(self):
        """-> [(allocation, side, first offset, last offset, bytes found at the two, number of bytes changed)]; offsets count from
        the interior's first byte (head: negative) or from the first byte behind it (tail: 0 = the byte right behind the interior)."""
        out = []
        for e in self.registry:
            b, g, n = e["backing"], e["guard"], e["nbytes"]
            for side, band, origin in (("head", b[:g], -g), ("tail", b[g + n:], 0)):
                bad = band != GUARD_BYTE
                if bool(bad.any().item()):
                    idx = bad.nonzero().flatten()
                    first, last = int(idx[0].item()), int(idx[-1].item())
                    out.append((_name(e), side, first + origin, last + origin, (int(band[first].item()), int(band[last].item())),
                                int(idx.numel())))
        return out

    def check(self):
        """After a synchronize: every guard byte of every registered buffer still holds GUARD_BYTE."""
        bad = self.violations()
        if bad:
            lines = [f"{name}: {side} guard, {count} bytes changed, offsets {first} .. {last} "
                     f"({'before the interior' if side == 'head' else 'behind the interior'}), found 0x{b0:02x} .. 0x{b1:02x}"
                     for name, side, first, last, (b0, b1), count in bad]
            raise GuardViolation("a store landed outside its buffer:\n  " + "\n  ".join(lines))


def _name(e):
    return f"{e['where']}: {e['fn']} {e['shape']} {str(e['dtype']).replace('torch.', '')}"


def _caller():
    f = sys._getframe(1)
    here = os.path.abspath(__file__)
    while f is not None and os.path.abspath(f.f_code.co_filename) == here:
        f = f.f_back
    return "?" if f is None else f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} {f.f_code.co_name}"


def _modules():
    import mocodad_amd.engine as engine
    import mocodad_amd.stream as stream
    return engine, stream


@contextlib.contextmanager
def guarded(**options):
    """Installs a GuardedTorch as `torch` of mocodad_amd.engine and mocodad_amd.stream only; the real module is back on exit,
    also when the body raises."""
    g = GuardedTorch(**options)
    saved = [(m, m.torch) for m in _modules()]
    try:
        for m, _ in saved:
            m.torch = g
        yield g
    finally:
        for m, t in saved:
            m.torch = t


def unwritten(t):
    """Elements of t that still hold the all-ones pattern an `empty` interior starts with."""
    if t.numel() == 0:
        return 0
    view = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}[t.element_size()]
    bits = t.contiguous().view(view)
    return int((bits == (POISON if view == _torch.uint8 else -1)).sum().item())


def guarded_copy(t, fill, seed=0):
    """t copied between two bands of max(GUARD, one row) bytes: all-ones NaNs (fill='nan') or finite random floats in (-1, 1)
    (fill='finite').  The result shares the backing tensor's storage, which lives as long as the result does."""
    if fill not in ("nan", "finite"):
        raise ValueError("fill: 'nan' or 'finite'")
    t = t.contiguous()
    nbytes = t.numel() * t.element_size()
    guard, _ = _guard_bytes(tuple(t.shape), t.element_size())
    if fill == "nan":
        backing = _torch.full((2 * guard + nbytes,), POISON, dtype=_torch.uint8, device=t.device)
    else:
        gen = _torch.Generator().manual_seed(seed)
        words = (2 * guard + nbytes + 3) // 4
        band = (_torch.rand(words, generator=gen) * 2 - 1).view(_torch.uint8)[:2 * guard + nbytes]
        backing = band.to(t.device).contiguous()
    out = backing[guard:guard + nbytes].view(t.dtype).view(t.shape)
    out.copy_(t)
    return out
