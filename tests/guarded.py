"""Guarded buffers for kernel tests: every result, operand and scratch region a kernel is handed lies inside a larger buffer that is
pre-filled, interior included, with one fixed bit pattern per element type.

  out(shape, dtype)      a result: after the call both guards must hold the pattern BIT FOR BIT (a NaN of the kernel's own in a guard
                         fails) and no interior element may still hold it (or exactly the elements of an `untouched=` mask);
  inp(array, dtype)      an operand: its surroundings hold the same pattern, so a read outside the operand that reaches a result shows as
                         a NaN or a wrong value in the test's own comparison;
  scratch(n, dtype)      exactly n elements of pattern (never zeros) between guards: what a region of the engine's arena looks like to the
                         kernel that gets it after another one;
  check(what)            one synchronisation, then the assertions above for everything handed out since the last check (results are
                         checked once; operands and scratch keep being watched until reset()).

The patterns: f32 0x7FC12345 (a quiet NaN no kernel here produces), 16-bit planes 0x7FC1 (NaN as bf16 and as fp16), f64
0x7FF8000012345679, uint8 255, int32 / int64 -0x12345679 (outside every legal range of a label, a count or an index).

A plain module (like first_block_ref.py): no fixtures, runs on device="cpu" as well (tests/test_guarded_cpu.py).
"""
import numpy as np
import torch

GUARD = 4096                        # elements; the least a guard is, on either side
DEVICE = "cuda:0"

F32_PATTERN = 0x7FC12345
H16_PATTERN = 0x7FC1
F64_PATTERN = 0x7FF8000012345679
U8_PATTERN = 255
INT_PATTERN = -0x12345679

# element type -> (integer type of the same width the bits are compared in, the pattern)
_BITS = {
    torch.float32: (torch.int32, F32_PATTERN),
    torch.float64: (torch.int64, F64_PATTERN),
    torch.float16: (torch.int16, H16_PATTERN),
    torch.bfloat16: (torch.int16, H16_PATTERN),
    torch.int16: (torch.int16, H16_PATTERN),
    torch.uint8: (torch.uint8, U8_PATTERN),
    torch.int32: (torch.int32, INT_PATTERN),
    torch.int64: (torch.int64, INT_PATTERN),
}


class _Buf:
    __slots__ = ("raw", "guard", "n", "t", "kind", "pat", "checked")

    def __init__(self, n, shape, dtype, guard, kind, device):
        assert guard >= GUARD, "a guard is at least %d elements" % GUARD
        idt, self.pat = _BITS[dtype]
        self.guard = (int(guard) + 15) // 16 * 16                     # the view stays 16-byte aligned whatever the element size
        self.n = int(n)
        self.raw = torch.full((2 * self.guard + self.n,), self.pat, dtype=idt, device=device)
        self.t = self.raw[self.guard:self.guard + self.n].view(dtype).view(tuple(shape))
        self.kind = kind
        self.checked = False

    def interior(self):
        return self.raw[self.guard:self.guard + self.n]

    def guard_damage(self):
        """number of guard elements that no longer hold the pattern (a tensor on the buffer's device)"""
        g = self.guard
        return (self.raw[:g] != self.pat).sum() + (self.raw[g + self.n:] != self.pat).sum()


_live = []          # every buffer handed out since reset(): keeps it allocated (kernels run asynchronously) and watched
_by_id = {}


def reset():
    """forget every buffer (start of a test)"""
    del _live[:]
    _by_id.clear()


def _register(b):
    _live.append(b)
    _by_id[id(b.t)] = b
    return b.t


def _record(t):
    b = _by_id.get(id(t))
    assert b is not None and b.t is t, "not a tensor handed out by guarded.out / inp / scratch"
    return b


def out(shape, dtype=torch.float32, guard=GUARD, device=None):
    """a result of this shape: poisoned, between two guards of `guard` elements each"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return _register(_Buf(int(np.prod(shape, dtype=np.int64)), shape, dtype, guard, "out", device or DEVICE))


def inp(array, dtype=torch.float32, guard=GUARD, device=None):
    """a copy of the operand between two guards of poison"""
    src = array if isinstance(array, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(array))
    src = src.to(dtype).contiguous()
    b = _Buf(src.numel(), src.shape, dtype, guard, "inp", device or DEVICE)
    b.t.copy_(src)
    return _register(b)


def scratch(n, dtype=torch.float32, guard=GUARD, device=None):
    """exactly n poisoned elements between two guards"""
    return _register(_Buf(n, (int(n),), dtype, guard, "scratch", device or DEVICE))


def whole(t):
    """the whole buffer around t, guards included, as t's element type; t starts at element offset(t)"""
    b = _record(t)
    return b.raw.view(t.dtype)


def offset(t):
    return _record(t).guard


def poisoned(t, part=None):
    """the elements of t (a guarded tensor, or with part= a slice / index of it taken by the caller) that hold the pattern, as a bool
    tensor"""
    b = _record(t)
    idt, pat = _BITS[t.dtype]
    v = t if part is None else part
    return v.contiguous().view(idt) == pat


def no_poison(t, part, what):
    """assert that `part` (a slice of the guarded tensor t) holds no element of the pattern: the rows a call reports back out of a scratch"""
    p = poisoned(t, part).reshape(-1)
    n = int(p.sum())
    assert n == 0, "%s: %d of %d reported elements were never written, first at %d" % (what, n, p.numel(), int(torch.nonzero(p)[0]))


def pending():
    """results handed out and not yet checked"""
    return [b.t for b in _live if b.kind == "out" and not b.checked]


def check(what, untouched=None):
    """Synchronise; every live buffer's guards must hold the pattern bit for bit; every result not checked before must hold the pattern
    nowhere, or — untouched=[(tensor, bool mask of its shape), ...] — exactly where its mask says."""
    masks = {}
    for t, m in (untouched.items() if isinstance(untouched, dict) else (untouched or [])):
        b = _record(t)
        assert b.kind == "out" and not b.checked
        m = torch.as_tensor(np.asarray(m) if not isinstance(m, torch.Tensor) else m).to(torch.bool)
        masks[id(t)] = torch.broadcast_to(m.to(b.raw.device), t.shape).reshape(-1)
    if _live and _live[0].raw.is_cuda:
        torch.cuda.synchronize()
    outs = [b for b in _live if b.kind == "out" and not b.checked]
    bad = None
    # the guards of every live buffer, compared in one pass per element type (a test with many calls has many live buffers)
    guards = {}
    for b in _live:
        guards.setdefault((b.raw.dtype, b.pat), []).extend((b.raw[:b.guard], b.raw[b.guard + b.n:]))
    for (_, pat), parts in guards.items():
        d = (torch.cat(parts) != pat).sum()
        bad = d if bad is None else bad + d
    for b in outs:
        kept = b.interior() == b.pat
        m = masks.get(id(b.t))
        d = kept.sum() if m is None else (kept != m).sum()
        bad = d if bad is None else bad + d
    for b in outs:
        b.checked = True
    if bad is None or int(bad) == 0:
        return
    # something is wrong: say what (the slow path)
    msgs = []
    for b in _live:
        if int(b.guard_damage()):
            g = b.guard
            lo = torch.nonzero(b.raw[:g] != b.pat).reshape(-1)
            hi = torch.nonzero(b.raw[g + b.n:] != b.pat).reshape(-1)
            msgs.append("%s wrote outside its %s %s of %d elements: %d elements in front (nearest %s before the start), %d behind (first "
                        "%s after the end)" % (what, b.kind, tuple(b.t.shape), b.n, lo.numel(), g - int(lo[-1]) if lo.numel() else "-",
                                               hi.numel(), int(hi[0]) if hi.numel() else "-"))
    for b in outs:
        kept = b.interior() == b.pat
        m = masks.get(id(b.t))
        if m is None:
            if int(kept.sum()):
                msgs.append("%s left %d of %d elements of its result %s unwritten, first at flat index %d"
                            % (what, int(kept.sum()), b.n, tuple(b.t.shape), int(torch.nonzero(kept)[0])))
        else:
            missed, over = kept & ~m, ~kept & m
            if int(missed.sum()):
                msgs.append("%s left %d elements of its result %s unwritten that it should write, first at flat index %d"
                            % (what, int(missed.sum()), tuple(b.t.shape), int(torch.nonzero(missed)[0])))
            if int(over.sum()):
                msgs.append("%s wrote %d elements of its result %s that it should leave alone, first at flat index %d"
                            % (what, int(over.sum()), tuple(b.t.shape), int(torch.nonzero(over)[0])))
    raise AssertionError("; ".join(msgs))
