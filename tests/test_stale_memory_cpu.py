"""The stale-memory helper itself (tests/stale_memory.py), on CPU tensors: the four patterns land in the buffer, the
record is complete, ``torch.zeros`` is untouched, ``torch.empty`` is restored on exit and after an exception, and the
check against vacuity fails when nothing was allocated.  tests/test_stale_memory_gpu.py relies on each of these."""
import numpy as np
import pytest
import torch

import stale_memory
from stale_memory import PATTERNS, StaleMemory, same

DTYPES = (torch.float32, torch.float64, torch.int32)


def _front_end(dtype):
    """What the package's front ends do: ``torch.empty`` looked up on the module at call time."""
    return torch.empty((3, 5), dtype=dtype), torch.empty(7, dtype=dtype, device="cpu"), torch.zeros((4,), dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_four_patterns_land_in_the_buffer(dtype):
    got = {}
    for pattern in PATTERNS:
        with StaleMemory(pattern, seed=3) as mem:
            a, b, z = _front_end(dtype)
        assert a.dtype == dtype and a.shape == (3, 5) and b.shape == (7,)
        assert not z.any()                                         # torch.zeros is untouched
        assert len(mem.records) == 2                               # ... and not recorded
        got[pattern] = (a, b)
    for t in got["zeros"]:
        assert not t.any()
    if dtype.is_floating_point:
        assert all(bool(torch.isnan(t).all()) for t in got["nan"])
        assert all(bool((t == float("inf")).all()) for t in got["inf"])
        for t in got["garbage"]:
            assert bool(torch.isfinite(t).all())
            assert bool((t.abs() >= 0.5e30).all()) and bool((t.abs() < 1.5e30).all())
        both = torch.cat([t.reshape(-1) for t in got["garbage"]])
        assert bool((both > 0).any()) and bool((both < 0).any())   # mixed signs
        assert both.unique().numel() > both.numel() // 2           # not one value
    else:
        assert all(bool((t == stale_memory.NAN_BITS).all()) for t in got["nan"])
        assert np.float32(np.nan).view(np.int32) == stale_memory.NAN_BITS
        assert all(bool((t == -1).all()) for t in got["inf"])     # all ones
        both = torch.cat([t.reshape(-1) for t in got["garbage"]])
        assert both.unique().numel() > both.numel() // 2
        assert bool((both < 0).any()) and bool((both > 0).any())   # the top bit is exercised too


def test_the_garbage_is_seeded():
    def draw(seed):
        with StaleMemory("garbage", seed=seed):
            return torch.empty(64), torch.empty(64)
    a, b = draw(1)
    c, d = draw(1)
    e, _ = draw(2)
    assert torch.equal(a, c) and torch.equal(b, d)
    assert not torch.equal(a, b) and not torch.equal(a, e)         # per allocation and per seed


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_record_is_complete(dtype):
    with StaleMemory("nan") as mem:
        a, b, _ = _front_end(dtype)
        c = torch.empty((0, 4), dtype=dtype)
    assert [r.data_ptr for r in mem.records] == [a.data_ptr(), b.data_ptr(), c.data_ptr()]
    assert [r.nbytes for r in mem.records] == [15 * a.element_size(), 7 * a.element_size(), 0]
    assert all(r.dtype == dtype and r.device == torch.device("cpu") for r in mem.records)
    mem.check(returned=dict(a=a, b=b, c=c), workspace_bytes=0)
    mem.check(returned=[a], workspace_bytes=7 * a.element_size())  # b serves as the workspace
    with pytest.raises(AssertionError, match="workspace"):
        mem.check(returned=[a, b], workspace_bytes=8)              # every buffer of that size is an output
    with pytest.raises(AssertionError, match="workspace"):
        mem.check(returned=[a], workspace_bytes=16 * a.element_size())
    with pytest.raises(AssertionError, match="not allocated under the patch"):
        mem.check(returned=dict(z=torch.zeros(3, dtype=dtype)))
    with pytest.raises(AssertionError, match="not allocated under the patch"):
        mem.check(returned=dict(tail=a.reshape(-1)[1:]))            # matched by data_ptr: an offset view is not it
    mem.check(returned=dict(view=a[0], flat=a.reshape(-1)))         # a view from the start is


def test_torch_empty_is_restored_on_exit_and_after_an_exception():
    real = torch.empty
    with StaleMemory("inf"):
        assert torch.empty is not real
    assert torch.empty is real
    with pytest.raises(RuntimeError, match="boom"):
        with StaleMemory("garbage"):
            assert torch.empty is not real
            raise RuntimeError("boom")
    assert torch.empty is real
    # nested uses unwind in order
    with StaleMemory("zeros") as outer:
        with StaleMemory("nan") as inner:
            t = torch.empty(3)
        u = torch.empty(3)
    assert torch.empty is real
    assert bool(torch.isnan(t).all()) and len(inner.records) == 1
    assert not u.any() and len(outer.records) == 2                  # the inner call goes through the outer one


def test_the_vacuity_check_fails_when_nothing_was_allocated():
    with StaleMemory("nan") as mem:
        torch.zeros(5)
    with pytest.raises(AssertionError, match="was not called under the patch"):
        mem.check()
    with pytest.raises(ValueError):
        StaleMemory("ones")


def test_same_is_nan_positions_and_bits():
    nan, inf = float("nan"), float("inf")
    for dtype in (torch.float32, torch.float64):
        a = torch.tensor([1.0, nan, -0.0, inf], dtype=dtype)
        assert same(a, a.clone())
        assert not same(a, torch.tensor([1.0, nan, 0.0, inf], dtype=dtype))                       # -0.0 is not 0.0
        assert not same(a, torch.tensor([1.0, nan, -0.0, torch.finfo(dtype).max], dtype=dtype))   # inf is not max
        assert not same(a, torch.tensor([nan, 1.0, -0.0, inf], dtype=dtype))
        assert not same(a, a[:3])
    one = torch.tensor([1.0 + 2.0 ** -40], dtype=torch.float64)
    assert not same(one, torch.ones(1, dtype=torch.float64))       # no pass through fp32
    assert not same(torch.ones(1), torch.ones(1, dtype=torch.float64))
    big = torch.tensor([2 ** 24 + 1, -1], dtype=torch.int32)
    assert same(big, big.clone()) and not same(big, torch.tensor([2 ** 24, -1], dtype=torch.int32))
    assert same(torch.tensor([True, False]), torch.tensor([True, False]))
    assert stale_memory._same is same


def test_autograd_hands_the_backward_buffers_through():
    """A gradient buffer that a Function's backward takes from ``torch.empty`` reaches ``.grad`` and
    ``torch.autograd.grad`` as the same memory: what lets the GPU cases match gradients by ``data_ptr``."""
    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.empty(x.shape, dtype=x.dtype)
            out.copy_(2 * x)
            return out

        @staticmethod
        def backward(ctx, g):
            out = torch.empty(g.shape, dtype=g.dtype)
            out.copy_(2 * g)
            return out

    x = torch.arange(6.0).reshape(2, 3).requires_grad_()
    with StaleMemory("nan") as mem:
        y = Twice.apply(x.reshape(2, 3, 1))
        y.sum().backward()
    assert torch.equal(x.grad, torch.full((2, 3), 2.0))
    mem.check(returned=dict(y=y, grad=x.grad))
