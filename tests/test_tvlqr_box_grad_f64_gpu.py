"""Double-precision gradients through the control-limited TV-LQR solve on the MI355X (tfmpc_tvlqr_box_vjp_f64 through
tfmpc.solvers.tvlqr_box_vjp(dtype=torch.float64) and tvlqr_box_solve(dtype=torch.float64, differentiable=True);
DESIGN.md 3.20) against the 80-bit value-form reference of tests/tvlqr_box_grad_f64_ref.py on the SAME trajectory and held
set, all seven-plus-two gradients, under its budget rule: per output and instance, kernel error over max(error of the fp64
restatement, 2^-48 max(1, |ref|)); the median over instances <= 2.5 and every instance <= 10; a batch- or time-summed
gradient's budget is the sum of its terms' budgets.  Outputs that are exactly zero by DESIGN.md 3.11 must be exactly zero.
tests/test_tvlqr_box_grad_f64_cpu.py asserts that every case here has 30 - 70 % of its controls held."""
import numpy as np
import pytest
import torch

import tvlqr_box_f64_ref as dref
import tvlqr_box_grad_f64_ref as bg
from tfmpc import _hip
from tfmpc.solvers import tvlqr_box_solve, tvlqr_box_vjp

pytestmark = pytest.mark.gpu

F64 = torch.float64
KEYS = {"F": "F", "f": "f", "C": "C", "c": "c", "x0": "x0", "low": "low", "high": "high", "C_final": "Cfin", "c_final": "cfin"}


def _dev(a, dtype=F64):
    return None if a is None else torch.as_tensor(np.asarray(a), device="cuda", dtype=dtype)


def _vjp(user, states, actions, w, dtype=F64):
    """tvlqr_box_vjp on what the caller passes -> (gradients as numpy under the reference's names, clamped, status)."""
    def op(k):                       # a vector of ONE entry per step carries its column axis, or [B, T, 1] reads as [T, 1, 1]
        t = _dev(user[k], dtype)
        return t.unsqueeze(-1) if k in ("f", "low", "high") and t.dim() >= 2 and t.shape[-1] == 1 else t

    got = tvlqr_box_vjp(*(op(k) for k in ("F", "f", "C", "c", "low", "high")), _dev(states, dtype), _dev(actions, dtype),
                        *(_dev(g, dtype) for g in w), C_final=_dev(user.get("Cfin"), dtype), c_final=_dev(user.get("cfin"), dtype),
                        dtype=dtype)
    torch.cuda.synchronize()
    out = {}
    for k, name in KEYS.items():
        if k in got:
            want = np.shape(user[name]) if name != "x0" else (states.shape[0], states.shape[2])
            if name in ("low", "high") and len(want) < 2:
                want = (1, actions.shape[2])                        # a scalar or [m] bound: one row of per-control sums
            assert got[k].dtype == dtype and tuple(got[k].shape) == tuple(want), (k, got[k].dtype, got[k].shape, want)
            out[name] = got[k].cpu().numpy()
    return out, got["clamped"].cpu().numpy(), got["status"].cpu().numpy()


def _run(what, loss="mixed", log=None, **kw):
    full, user, states, actions, held, w, refs = bg.case(loss=loss, **kw)
    got, clamped, status = _vjp(user, states, actions, w)
    assert not status.any() and np.array_equal(clamped, held), (what, status)
    B, T, m = actions.shape
    shared = tuple(k for k in got if _batch_summed(k, user, full))
    timed = tuple(k for k in got if _time_summed(k, user, full, T))
    bg.check(got, refs, what=what, shared=shared, time_shared=timed, log=log)
    at_low = held & (actions == np.broadcast_to(full["low"], actions.shape))
    zeros = bg.exact_zeros(got, held, at_low, states.shape[2], loss, summed=set(shared) | set(timed))
    return got, zeros


def _batch_summed(k, user, full):
    if k == "x0":
        return False
    if k in ("low", "high"):
        return np.ndim(user[k]) < 3
    return np.ndim(user[k]) < np.ndim(full[k])


def _time_summed(k, user, full, T):
    if k not in bg.TIMED or T == 1:
        return False
    if k in ("low", "high"):
        return np.ndim(user[k]) < 2 or np.shape(user[k])[-2] == 1
    return np.shape(user[k])[1 - np.ndim(full[k])] == 1                               # the time axis, counted from the end


def _id(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items() if k not in ("shared", "const")) + ("-shared" if kw.get("shared") else "") + \
        ("-const" if kw.get("const") else "")


# ---- shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", bg.SHAPES + bg.FINAL + bg.ALL_HELD, ids=_id)
def test_shapes(kw):
    """The 16 -> 32 switch in each dimension, all 32 mask bits (bit 31 included), every control held, an explicit final
    cost per instance and shared."""
    _run(f"shapes {_id(kw)}", **kw)


@pytest.mark.parametrize("kw", bg.NONE_HELD, ids=_id)
def test_no_control_held_is_the_plain_double_vjp_bit_for_bit(kw):
    """Bounds at +-inf and at +-1e6: every gradient has the bits of tfmpc_tvlqr_vjp_f64 on the same trajectory with the v of
    tfmpc_tvlqr_solve_f64 on the same operands; dlow and dhigh are exact zeros."""
    full, user, states, actions, held, w, _ = bg.case(**kw)
    assert not held.any()
    got, clamped, status = _vjp(user, states, actions, w)
    assert not status.any() and not clamped.any()
    assert (got["low"] == 0).all() and (got["high"] == 0).all() and not np.signbit(got["low"]).any()
    lib = _hip.load()
    B, T, m = actions.shape
    n, d = states.shape[2], states.shape[2] + m
    t = {k: _dev(user[k]) for k in ("F", "f", "C", "c", "x0")}
    xs, us, cs, v = (torch.empty(s, device="cuda", dtype=F64) for s in ((B, T + 1, n), (B, T, m), (B, T + 1), (B, T, n)))
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    model = [_hip.ptr(t["F"]), T * n * d, n * d, _hip.ptr(t["f"]), T * n, n, _hip.ptr(t["C"]), T * d * d, d * d, _hip.ptr(t["c"]), T * d, d,
             None, 0, None, 0]
    ws = torch.empty(int(lib.tfmpc_tvlqr_workspace_bytes_f64(B, n, m, T)) // 8 + 1, device="cuda", dtype=F64)
    rc = lib.tfmpc_tvlqr_solve_f64(B, n, m, T, *model, _hip.ptr(t["x0"]), _hip.ptr(xs), _hip.ptr(us), _hip.ptr(cs), None, None, None,
                                   _hip.ptr(v), None, _hip.ptr(st), _hip.ptr(ws), ws.numel() * 8, None)
    assert rc == 0
    outs = {k: torch.empty_like(t[k]) for k in ("F", "f", "C", "c")}
    dx0 = torch.empty(B, n, device="cuda", dtype=F64)
    ws = torch.empty(int(lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(B, n, m, T)) // 8 + 1, device="cuda", dtype=F64)
    g = [_dev(a) for a in w]
    traj = (_dev(states), _dev(actions))                          # (kept alive across the launch)
    rc = lib.tfmpc_tvlqr_vjp_f64(B, n, m, T, *model, _hip.ptr(traj[0]), _hip.ptr(traj[1]), _hip.ptr(v), *(_hip.ptr(a) for a in g),
                                 _hip.ptr(outs["F"]), T * n * d, n * d, _hip.ptr(outs["f"]), T * n, n, _hip.ptr(outs["C"]), T * d * d, d * d,
                                 _hip.ptr(outs["c"]), T * d, d, None, 0, None, 0, _hip.ptr(dx0), n, _hip.ptr(st), _hip.ptr(ws),
                                 ws.numel() * 8, None)
    torch.cuda.synchronize()
    assert rc == 0 and not st.any()
    outs["x0"] = dx0
    for k, a in outs.items():
        a = a.cpu().numpy()
        print(f"none held d{k}: {int((got[k] != a).sum())} of {a.size} entries differ, by at most {np.abs(got[k] - a).max():.3g}")
        assert np.array_equal(got[k], a), k


# ---- sharing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", bg.LOSSES)
@pytest.mark.parametrize("kw", bg.SHARED, ids=_id)
def test_shared_operands_bounds_and_losses(kw, loss):
    _run(f"sharing {_id(kw)} {loss}", loss=loss, **kw)


@pytest.mark.parametrize("kw", bg.BOUND_FORMS, ids=_id)
def test_every_form_of_the_bounds(kw):
    """scalar, [m], [T, m], [B, 1, m] (time-accumulated per instance) and [B, T, m]."""
    _run(f"bounds {_id(kw)}", **kw)


@pytest.mark.parametrize("loss", ["states", "actions"])
@pytest.mark.parametrize("kw", bg.ZEROS, ids=_id)
def test_exact_zeros_under_a_loss_without_a_cost_term(kw, loss):
    """Nothing shared, bounds [B, T, m]: dc[n + i] of a held control and the dC entries between two held controls are exact
    zeros, as are dlow / dhigh off the held set and on the other bound -- all four checks run."""
    _, zeros = _run(f"zeros {_id(kw)} {loss}", loss=loss, **kw)
    assert zeros == {"low", "high", "c", "C"}


@pytest.mark.parametrize("kw", bg.CHUNKS, ids=_id)
def test_shared_bounds_across_chunk_edges_and_twice_the_same_bits(kw):
    got, _ = _run(f"chunks {_id(kw)}", **kw)
    again, _ = _run(f"chunks {_id(kw)} again", **kw)
    for k in got:
        assert np.isfinite(got[k]).all() and np.array_equal(got[k], again[k]), k


# ---- what the value-function costates buy -----------------------------------------------------------------------------

def test_unscaled_model_at_the_headline_horizon():
    """rho(F_x) ~ 5 over T = 50 with about half of the controls held: the rule holds, and the fp32 box VJP on the same
    numbers is at least 1e4 times worse on dF, df, dx0 -- by a FINITE error in at least one instance, so that an fp32 path
    which returned NaN for another reason would not pass."""
    full, user, states, actions, held, w, refs = bg.case(unscaled=True)
    got, clamped, status = _vjp(user, states, actions, w)
    assert not status.any() and np.array_equal(clamped, held)
    bg.check(got, refs, what="unscaled (16, 8, 50)")
    got32, _, _ = _vjp(user, states, actions, w, dtype=torch.float32)
    for k in ("F", "f", "x0"):
        finite = 0
        for b in range(actions.shape[0]):
            e64, e32 = bg._err(got[k][b], refs[0][k][b]), bg._err(got32[k][b], refs[0][k][b])
            finite += bool(np.isfinite(e32))
            e32 = e32 if np.isfinite(e32) else np.inf
            print(f"unscaled d{k}[{b}]: fp64 error {e64:.3g}, fp32 error {e32:.3g}, gain {e32 / max(e64, 1e-300):.3g}")
            assert e64 * 1e4 <= e32, (k, b, e64, e32)
        assert finite, k


def _device_forward(ops, differentiable=False, **kw):
    t = {k: _dev(v) for k, v in ops.items() if v is not None and k in ("F", "f", "C", "c", "x0", "low", "high")}
    if differentiable:
        for v in t.values():
            v.requires_grad_()
    out = tvlqr_box_solve(t["F"], t["f"], t["C"], t["c"], t["x0"], t["low"], t["high"], dtype=F64, differentiable=differentiable, **kw)
    return t, out


def _check_on_device_trajectory(what, ops, grads, out, w, pick=None):
    """The rule against the closed form on the DEVICE's trajectory and held set."""
    states, actions = out[0][..., 0].detach().cpu().numpy(), out[1][..., 0].detach().cpu().numpy()
    held = dref.held_from_actions(actions, ops["low"], ops["high"])
    refs = bg.references(ops, states, actions, held, *w)
    bg.check(grads, refs, what=what, idx=pick)
    return held


@pytest.mark.parametrize("rho,width", dref.RESCUED)
def test_the_rescued_class(rho, width):
    """DESIGN.md 3.18's instances that fp32 flags NOT_PD, on the device's own double forward: finite gradients, status 0,
    within the rule.  The class is made by bounds so tight that V grows along stretches where every control is held: at
    (1.35, 0.02) EVERY control of every instance is held (tests/test_tvlqr_box_grad_f64_cpu.py pins it on the fp64
    restatement), so the 30 - 70 % of the other cases cannot hold here; (1.25, 0.05) has held and free controls in one
    instance."""
    ops = dref.rescued_operands(rho, width)
    with torch.no_grad():
        _, out = _device_forward(ops)
    assert not out.info.last_status.any()
    states, actions = out[0][..., 0].cpu().numpy(), out[1][..., 0].cpu().numpy()
    B, T, m = actions.shape
    w = bg.weights(B, states.shape[2], m, T, "mixed")
    got, clamped, status = _vjp(ops, states, actions, w)
    assert not status.any() and all(np.isfinite(a).all() for a in got.values())
    held = _check_on_device_trajectory(f"rescued ({rho}, {width})", ops, got, out, w)
    print(f"rescued ({rho}, {width}): {held.mean():.3f} of the controls held")
    assert np.array_equal(clamped, held)
    if (rho, width) == dref.RESCUED[0]:
        assert held.all()
    else:
        mixed = held.reshape(B, -1)
        assert (mixed.any(1) & ~mixed.all(1)).any()


@pytest.mark.parametrize("kw", bg.END_TO_END, ids=_id)
def test_end_to_end(kw):
    full, user, _, _, _ = bg.forward_case(**kw)
    with torch.no_grad():
        _, plain = _device_forward(user)
    t, out = _device_forward(user, differentiable=True)
    assert all(a.dtype == F64 and a.requires_grad for a in out)
    for a, b in zip(plain, out):
        assert torch.equal(a, b.detach())
    B, T, m = out[1].shape[:3]
    w = bg.weights(B, out[0].shape[2], m, T, "mixed")
    loss = sum((o.reshape(g.shape) * _dev(g)).sum() for o, g in zip(out, w))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu().numpy() for k, v in t.items()}
    for k, v in t.items():
        assert v.grad.dtype == F64 and v.grad.shape == v.shape, k
    assert not out.info.last_grad_status.any()
    _check_on_device_trajectory(f"end to end {_id(kw)}", full, grads, out, w)


def test_gradcheck():
    """torch's default tolerances and step.  tests/test_tvlqr_box_grad_f64_cpu.py asserts that every multiplier and slack of
    this case exceeds 1e-2, so no difference step crosses a change of the held set."""
    full, user, _, _, _ = bg.forward_case(**bg.GRADCHECK)
    sym = lambda A: 0.5 * (A + A.transpose(-1, -2))                                      # noqa: E731
    ops = [_dev(user[k]).requires_grad_() for k in ("F", "f", "c", "x0", "low", "high", "C")]

    def fn(F, f, c, x0, low, high, A):
        return tuple(tvlqr_box_solve(F, f, sym(A), c, x0, low, high, dtype=F64, differentiable=True))

    assert torch.autograd.gradcheck(fn, ops)


# ---- status and degenerate inputs ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,bad", [(3, 1), (519, 300)])
def test_not_pd_instance(B, bad):
    """C per instance (one indefinite), the rest of the model shared: NaN in the instance's own rows, dlow / dhigh included,
    and in every batch sum; the other rows within the rule."""
    n, m, T = 4, 2, 2
    full, user, states, actions, held, w, refs = bg.case(**next(kw for kw in bg.NOT_PD if kw["B"] == B))
    user = dict(user, C=user["C"].copy())
    user["C"][bad, T - 1, n:, n:] = -1.0e4 * np.eye(m)
    actions = actions.copy()
    actions[bad] = 0.0                                            # free controls: the indefinite block stays in the masked model
    got, clamped, status = _vjp(user, states, actions, w)
    others = [b for b in range(B) if b != bad]
    assert status[bad] & _hip.ST_NOT_PD and (status[others] == 0).all(), status[bad]
    for k in ("F", "f"):
        assert np.isnan(got[k]).all(), k
    for k in ("C", "c", "x0", "low", "high"):
        assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][others]).all(), k
    bg.check({k: got[k] for k in ("C", "c", "x0", "low", "high")}, refs, what=f"not_pd B={B}", time_shared=("low", "high"), idx=others)


def test_an_empty_batch():
    n, m, T = 16, 8, 4
    z = lambda *s: torch.zeros(s, device="cuda", dtype=F64)                              # noqa: E731
    got = tvlqr_box_vjp(z(0, T, n, n + m), z(0, T, n), z(0, T, n + m, n + m), z(0, T, n + m), z(m), z(m), z(0, T + 1, n), z(0, T, m),
                        dtype=F64)
    torch.cuda.synchronize()
    assert got["F"].shape == (0, T, n, n + m) and got["F"].dtype == F64 and got["low"].shape == (1, m) and float(got["low"].abs().sum()) == 0.0
