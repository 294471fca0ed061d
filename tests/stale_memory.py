"""TEST INFRASTRUCTURE ONLY -- stale memory on demand: a context manager that replaces ``torch.empty`` with a function
that calls the real one, fills the result with a chosen pattern and records ``(data_ptr, nbytes, dtype, device)``.

Every front end of this package takes its workspace, its outputs and its gradient buffers from ``torch.empty`` by
attribute lookup at call time, so under the patch a kernel that forgets to write an element, or reads one nobody wrote,
meets the pattern in place of whatever the caching allocator happened to hand back (memory straight from the driver is
often zero).  ``torch.zeros`` is left alone: the arrays the front ends allocate with it keep their contract.

Patterns, in the order the tests run them (:data:`PATTERNS`):

====================  ====================================  ===========================================
pattern               floating-point buffers                integer buffers
====================  ====================================  ===========================================
``zeros``             0                                     0
``nan``               quiet NaN                             the bit pattern of a float NaN, 0x7fc00000
``inf``               +inf                                  all ones
``garbage``           seeded, finite, about 1e30, mixed     a seeded bit pattern
                      signs
====================  ====================================  ===========================================

The finite garbage matters because NaN is swallowed by fmax-style reductions and by every ``>`` acceptance test; a
large finite stale value is not.  Boolean buffers get False, True, True and an alternating pattern.

:func:`same` is the comparison of tests/test_workspace_independence_gpu.py made exact for every dtype: equal NaN
positions and equal bits elsewhere.  :meth:`StaleMemory.check` is the check against vacuity: a case in which the patch
was not hit fails rather than passes.
"""

import collections
from unittest import mock

import torch

PATTERNS = ("zeros", "nan", "inf", "garbage")
NAN_BITS = 0x7FC00000

Allocation = collections.namedtuple("Allocation", "data_ptr nbytes dtype device")

_BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _wrap(value, dtype):
    """``value``'s low bits as a number of the integer ``dtype``."""
    info = torch.iinfo(dtype)
    value &= (1 << info.bits) - 1
    if info.min < 0 and value >= 1 << (info.bits - 1):
        value -= 1 << info.bits
    return value


def _hash(numel, seed, device):
    """A seeded, position-dependent 31-bit word per element (Knuth's multiplicative hash), int64."""
    idx = torch.arange(numel, device=device, dtype=torch.int64)
    return ((idx + 1 + 7919 * seed) * 2654435761 >> 5) & 0x7FFFFFFF


def fill(t, pattern, seed=0):
    """Fill ``t`` in place with ``pattern`` (see the module docstring)."""
    if pattern not in PATTERNS:
        raise ValueError(f"pattern must be one of {PATTERNS}, got {pattern!r}")
    if t.numel() == 0:
        return t
    if t.is_complex():
        fill(torch.view_as_real(t), pattern, seed)
    elif t.is_floating_point():
        if pattern == "garbage":
            h = _hash(t.numel(), seed, t.device)
            big = min(1e30, torch.finfo(t.dtype).max / 16)
            mag = (0.5 + (h & 0xFFFFF).to(torch.float64) / 0x100000) * big          # [0.5, 1.5) big
            t.copy_(torch.where((h >> 21 & 1).bool(), -mag, mag).reshape(t.shape))
        else:
            t.fill_({"zeros": 0.0, "nan": float("nan"), "inf": float("inf")}[pattern])
    elif t.dtype == torch.bool:
        if pattern == "garbage":
            t.copy_((_hash(t.numel(), seed, t.device) >> 9 & 1).bool().reshape(t.shape))
        else:
            t.fill_(pattern != "zeros")
    else:
        if pattern == "garbage":
            h = _hash(t.numel(), seed, t.device)
            info = torch.iinfo(t.dtype)
            h = (h | (h << 31)) & ((1 << info.bits) - 1) if info.bits < 64 else h | (h << 31)
            if info.bits < 64 and info.min < 0:
                h = torch.where(h >= 1 << (info.bits - 1), h - (1 << info.bits), h)
            t.copy_(h.reshape(t.shape))
        else:
            t.fill_(_wrap({"zeros": 0, "nan": NAN_BITS, "inf": -1}[pattern], t.dtype))
    return t


class StaleMemory:
    """``with StaleMemory("nan") as mem: ...`` -- inside, every ``torch.empty`` result is pre-filled and recorded in
    ``mem.records``; on exit (also after an exception) ``torch.empty`` is the real one again.  Built on
    ``unittest.mock.patch.object``; no ``conftest.py`` involved."""

    def __init__(self, pattern, seed=0):
        if pattern not in PATTERNS:
            raise ValueError(f"pattern must be one of {PATTERNS}, got {pattern!r}")
        self.pattern, self.seed = pattern, seed
        self.records = []
        self._patch = None

    def __enter__(self):
        real = torch.empty

        def empty(*args, **kwargs):
            t = real(*args, **kwargs)
            fill(t, self.pattern, self.seed + len(self.records))
            self.records.append(Allocation(t.data_ptr(), t.numel() * t.element_size(), t.dtype, t.device))
            return t

        self._patch = mock.patch.object(torch, "empty", empty)
        self._patch.start()
        return self

    def __exit__(self, *exc):
        self._patch.stop()
        self._patch = None
        return False

    def check(self, returned=(), workspace_bytes=0):
        """The check against vacuity, called after the patched call.  ``returned``: the tensors (a dict by name, or a
        sequence) that the front end creates with ``torch.empty`` and hands back -- each must be a recorded allocation,
        matched by ``data_ptr``, dtype and device.  ``workspace_bytes``: the family's ``*_workspace_bytes`` for the
        case; where nonzero, a filled buffer of at least that size that is none of ``returned`` was handed out."""
        assert self.records, "torch.empty was not called under the patch: the case checks nothing"
        items = list(returned.items()) if isinstance(returned, dict) else list(enumerate(returned))
        theirs = set()
        for name, t in items:
            hit = [r for r in self.records if r.data_ptr == t.data_ptr() and r.dtype == t.dtype and r.device == t.device
                   and r.nbytes >= t.numel() * t.element_size()]
            assert hit or t.numel() == 0, f"returned tensor {name!r} was not allocated under the patch"
            theirs.add(t.data_ptr())
        if workspace_bytes:
            assert any(r.nbytes >= workspace_bytes and r.data_ptr not in theirs for r in self.records), \
                f"no pre-filled buffer of at least {workspace_bytes} bytes (the workspace) was handed out"


def same(a, b):
    """Equal dtype and shape, equal NaN positions and equal bits elsewhere (-0.0 is not 0.0, +inf is not the largest
    finite number; the payload of a NaN is not compared)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    bits = _BITS[a.element_size()]
    zero = torch.zeros((), dtype=a.dtype, device=a.device)
    return torch.equal(torch.where(na, zero, a).contiguous().view(bits), torch.where(nb, zero, b).contiguous().view(bits))


_same = same
