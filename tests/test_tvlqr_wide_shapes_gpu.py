"""The wave-per-instance time-varying LQR (tvlqr_generic.hip: tvlqr_wave.h over wave_ops.h) past 64 columns (``-m gpu``).
It shares wave_for_2d, the matrix-core product and the unpivoted elimination with the LQR wave kernel, and reloads the model
every step: its load_matrix runs with cols > 64 T times.  Shapes (49, 16), (56, 24), (70, 4), (8, 66) at T = 3, B = 3
(what each reaches: tests/wide_shapes_ref.py).

Through the C ABI into NaN-filled buffers with a guard row behind the batch and a guard behind status.  Models from
tvlqr_ref.make_models, compared against tvlqr_ref.solve in fp64 and fp32 under the rule of test_tvlqr_gpu.py: per instance
|gpu - fp64| / max(|fp32 restatement - fp64|, 1e-6 max(1, scale)), median <= 2.5 and every instance <= 10.
"""

import functools

import numpy as np
import pytest
import torch

import tvlqr_ref
from tfmpc import _hip

pytestmark = pytest.mark.gpu

FIELDS = ("states", "actions", "costs", "K", "k", "V", "v", "const")
SHAPES = [(49, 16), (56, 24), (70, 4), (8, 66)]
T, B = 3, 3


@functools.lru_cache(maxsize=None)
def _case(n, m):
    """Models [B, T, ...], initial states and the fp64 / fp32 restatements per instance, made once per shape."""
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=n * 100 + m)
    x0 = tvlqr_ref.make_x0(n, B)
    r64 = [tvlqr_ref.solve(F[b], f[b], C[b], c[b], x0[b], dtype=np.float64) for b in range(B)]
    r32 = [tvlqr_ref.solve(F[b], f[b], C[b], c[b], x0[b], dtype=np.float32) for b in range(B)]
    for a in (F, f, C, c, x0):
        a.setflags(write=False)
    return (F, f, C, c, x0), r64, r32


def _launch(model, split=False, time_constant=False):
    """The model's B instances in one fused solve with policy and value outputs, or one backward and one forward launch.
    ``time_constant``: operands [B, 1, ...] passed with time stride 0.  Returns ({key: [B, rows, width]}, status[B])."""
    lib = _hip.require_gpu()
    F, f, C, c, x0 = (torch.as_tensor(np.array(a, dtype=np.float32), device="cuda") for a in model)       # (a writable copy)
    nb, nt, n, d = F.shape
    m = d - n
    assert nb == B and nt == (1 if time_constant else T)
    assert lib.tfmpc_tvlqr_kernel_name(n, m, T) == b"tv_generic_wave"
    margs = [B, n, m, T]
    for t in (F, f, C, c):
        margs += [_hip.ptr(t), t.stride(0), 0 if time_constant else t.stride(1)]
    margs += [None, 0, None, 0]
    rows = dict(states=(T + 1, n), actions=(T, m), costs=(T + 1, 1), K=(T, m * n), k=(T, m), V=(T, n * n), v=(T, n), const=(T, 1))
    flat = {key: torch.full((B * r + 1, w), float("nan"), device="cuda") for key, (r, w) in rows.items()}
    status = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    p = lambda key: _hip.ptr(flat[key])                        # noqa: E731
    if split:
        rc = lib.tfmpc_tvlqr_backward_f32(*margs, p("K"), p("k"), p("V"), p("v"), p("const"), _hip.ptr(status), _hip.stream())
        assert rc == 0, ("tfmpc_tvlqr_backward_f32", rc)
        rc = lib.tfmpc_tvlqr_forward_f32(*margs, p("K"), T * m * n, p("k"), T * m, _hip.ptr(x0), p("states"), p("actions"),
                                         p("costs"), _hip.stream())
        assert rc == 0, ("tfmpc_tvlqr_forward_f32", rc)
    else:
        rc = lib.tfmpc_tvlqr_solve_f32(*margs, _hip.ptr(x0), p("states"), p("actions"), p("costs"), p("K"), p("k"), p("V"),
                                       p("v"), p("const"), _hip.ptr(status), None, 0, _hip.stream())
        assert rc == 0, ("tfmpc_tvlqr_solve_f32", rc)
    torch.cuda.synchronize()
    out = {}
    for key, (r, w) in rows.items():
        assert torch.isnan(flat[key][B * r:]).all(), ((n, m), key, "guard row behind the batch")
        out[key] = flat[key][:B * r].reshape(B, r, w)
    assert int(status[B]) == -1, ((n, m), "guard behind the status")
    st = status[:B]
    assert int((st < 0).sum()) == 0, ((n, m), "a status nobody wrote", st.tolist())
    for key in out:
        assert torch.isfinite(out[key][st == 0]).all(), ((n, m), key, "an element inside the batch is not finite")
    return out, st


def _check(out, r64, r32, what):
    for key in FIELDS:
        got = out[key].cpu().numpy().astype(np.float64)
        ratios = []
        for b in range(B):
            ref = r64[b][key]
            scale = max(1.0, float(np.abs(ref).max()))
            budget = max(float(np.abs(r32[b][key] - ref).max()), 1e-6 * scale)
            ratios.append(float(np.abs(got[b].reshape(ref.shape) - ref).max()) / budget)
        print(f"{what} {key}: median {np.median(ratios):.2f} max {max(ratios):.2f}")
        assert np.median(ratios) <= 2.5 and max(ratios) <= 10.0, (what, key, np.median(ratios), max(ratios))


def _same_bits(got, want, what):
    for key in FIELDS:
        assert torch.equal(got[0][key], want[0][key]), (what, key)
    assert torch.equal(got[1], want[1]), (what, "status")


@pytest.mark.parametrize("n,m", SHAPES)
def test_fused_solve_against_the_restatement_and_split_equals_fused(n, m):
    model, r64, r32 = _case(n, m)
    for r in r32:                                              # the budget's denominator exists at this shape
        assert all(np.isfinite(r[key]).all() for key in FIELDS), (n, m)
    fused = _launch(model)
    assert fused[1].tolist() == [0] * B
    _check(fused[0], r64, r32, f"tv ({n}, {m})")
    _same_bits(_launch(model, split=True), fused, ((n, m), "backward + forward against fused"))


@pytest.mark.parametrize("n,m", SHAPES)
def test_time_stride_zero_gives_the_bits_of_the_repeated_model(n, m):
    F, f, C, c, x0 = _case(n, m)[0]
    once = tuple(a[:, :1] for a in (F, f, C, c)) + (x0,)
    repeated = tuple(np.repeat(a[:, :1], T, axis=1) for a in (F, f, C, c)) + (x0,)
    constant = _launch(once, time_constant=True)
    assert constant[1].tolist() == [0] * B
    _same_bits(constant, _launch(repeated), ((n, m), "time stride 0 against the repeated model"))


@pytest.mark.parametrize("n,m", SHAPES)
def test_not_pd_at_one_step_of_one_instance(n, m):
    F, f, C, c, x0 = _case(n, m)[0]
    C = C.copy()
    C[1, 1, n:, n:] = -1.0e4 * np.eye(m, dtype=np.float32)
    good = _launch(_case(n, m)[0])
    out, status = _launch((F, f, C, c, x0))
    assert int(status[1]) & _hip.ST_NOT_PD, status.tolist()
    assert int(status[0]) == 0 and int(status[2]) == 0, status.tolist()
    for key in FIELDS:                                         # the neighbours are untouched by it
        for b in (0, 2):
            assert torch.equal(out[key][b], good[0][key][b]), ((n, m), key, b)
