"""No result of the newer solver families may depend on what their workspace, output or gradient buffers held before
the call (the rule of tests/test_workspace_independence_gpu.py, which covers iLQR.solve_device and LQR.solve_device).

Every front end of these families takes its workspace, its outputs and its gradient buffers from ``torch.empty`` at call
time; tests/stale_memory.py replaces it with one that pre-fills what it hands out.  Each case runs the same call under
zeros, quiet NaN, +inf and seeded finite garbage of about 1e30 (zeros first), requires every returned tensor to be
identical -- equal NaN positions, equal bits elsewhere -- across the fills and in a fifth, unpatched call, and asserts
that the patch was hit: a pre-filled buffer of at least the family's ``*_workspace_bytes`` was handed out and every
returned tensor the front end creates with ``torch.empty`` is a recorded allocation.  Where ``solve_device(workspace=)``
exists, one caller-owned workspace pre-filled in place is passed as well.  No tolerance is involved: the reference of
every assertion is the call's own bits under another fill.

Shapes are the smallest that select each kernel variant (the ``*_kernel_name`` exports, asserted); B = 3, T = 5 unless a
family needs otherwise, B = 257 where a second reduction chunk holding one instance matters.  ``flagged``: instance 1's
R block of one middle step is -1e3 I; its NaN rows and its neighbours' bits must not move either.

Families: tfmpc_tvlqr_{solve,backward,forward}_f32 / _f64, tfmpc_tvlqr_solve_time_parallel_f64, tfmpc_tvlqr_vjp_f32 /
_f64, tfmpc_tvlqr_backward_vjp_f32, tfmpc_tvlqr_box_vjp_f32 / _f64, tfmpc_tvlqr_box_solve_f32 / _f64,
tfmpc_lqr_steady_state_f32 / _f64 and tfmpc_lqr_steady_state_vjp_f32."""
import functools

import numpy as np
import pytest
import torch

import lqr_box_grad_ref as bref
import lqr_steady_state_ref as ssref
import tvlqr_backward_grad_ref as bwref
import tvlqr_ref
import tvlqr_time_parallel_ref as tp
from stale_memory import PATTERNS, StaleMemory, fill, same
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR, lqr_steady_state, tvlqr_box_solve, tvlqr_box_vjp
from tfmpc.solvers.lqr import LQR

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
MODEL = ("F", "f", "C", "c")
LOSSES = ("states", "actions", "costs", "mixed")
INF = float("inf")


def _lib():
    return _hip.load()


def _dev(a, dtype):
    if a is None:
        return None
    a = np.asarray(a)                                              # (a scalar bound stays 0-d)
    return torch.as_tensor(np.ascontiguousarray(a) if a.ndim else a, device="cuda", dtype=dtype)


def _name(fn, *args):
    return getattr(_lib(), fn)(*args).decode()


def _snapshot(tensors):
    return {k: v.detach().clone() for k, v in tensors.items()}


def _run(call, workspace_bytes=0, what=""):
    """``call()`` -> (returned tensors by name, the names among them that the front end creates with ``torch.empty``).
    Runs it under the four fills, zeros first, and once unpatched; asserts the patch was hit and that every tensor is the
    same under all five.  Returns the zeros run's tensors."""
    runs = []
    for i, pattern in enumerate(PATTERNS):
        with StaleMemory(pattern, seed=17 * i) as mem:
            tensors, made = call()
            torch.cuda.synchronize()
        mem.check({k: tensors[k] for k in made}, workspace_bytes)
        runs.append(_snapshot(tensors))
    tensors, _ = call()
    torch.cuda.synchronize()
    runs.append(_snapshot(tensors))
    for label, other in zip(PATTERNS[1:] + ("unpatched",), runs[1:]):
        assert other.keys() == runs[0].keys()
        for k in runs[0]:
            assert same(runs[0][k], other[k]), (what, k, label)
    return runs[0]


@functools.lru_cache(maxsize=None)
def _pool(n, m, T, double, final, seed):
    """At most four distinct seeded models (the family tests' generators), read-only: F f C c Cfin cfin."""
    if double:
        F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, 4, seed=seed)
    else:
        F, f, C, c = tvlqr_ref.make_models(n, m, T, 4, seed=seed)
    Cf, cf = tvlqr_ref.make_final(n, 4, seed=seed + 1) if final else (None, None)
    return dict(F=F, f=f, C=C, c=c, Cfin=Cf, cfin=cf)


def _problem(n, m, T, B, dtype, final=None, shared=(), const=(), x0_shared=False, flagged=False, seed=0):
    """Operands as the caller passes them, numpy: the pool tiled to ``B`` instances, a distinct x0 per instance.
    ``shared``: no batch axis (instance 0's); ``const``: a time axis of 1 (step 0's); ``final``: None, "per" or "shared".
    ``flagged``: instance 1's R block at a middle step is -1e3 I (C must keep its batch axis)."""
    pool = _pool(n, m, T, dtype == F64, final is not None, seed + 100 * n + m)
    idx = np.arange(B) % 4
    ops = {k: pool[k][idx] for k in MODEL}
    if flagged:
        assert "C" not in shared and B > 1
        ops["C"] = ops["C"].copy()
        ops["C"][1, 0 if "C" in const else T // 2, n:, n:] = -1.0e3 * np.eye(m)
    for k in MODEL:
        a = ops[k][:, :1] if k in const else ops[k]
        ops[k] = np.ascontiguousarray(a[0] if k in shared else a)
    x0 = tvlqr_ref.make_x0(n, B, seed=seed + 2)
    ops["x0"] = x0[0].copy() if x0_shared else x0
    if final is not None:
        ops["Cfin"], ops["cfin"] = (pool[k][0].copy() if final == "shared" else pool[k][idx] for k in ("Cfin", "cfin"))
    return ops


def _tv(ops, dtype, leaves=False):
    """-> (TimeVaryingLQR, x0 [B, n, 1] or [n, 1], the tensors by name).  Vectors carry their column axis."""
    t = {k: _dev(v, dtype) for k, v in ops.items()}
    for k in ("f", "c", "x0", "cfin"):
        if t.get(k) is not None:
            t[k] = t[k].unsqueeze(-1)
    if leaves:
        for v in t.values():
            v.requires_grad_()
    tv = TimeVaryingLQR(t["F"], t["f"], t["C"], t["c"], t.get("Cfin"), t.get("cfin"), device="cuda", dtype=dtype)
    return tv, t["x0"], t


def _expect_flag(out, flagged, status="status", rows=("states", "actions", "costs")):
    st = out[status].cpu().numpy()
    if not flagged:
        assert not st.any(), st
        return
    assert st[1] != 0 and not np.delete(st, 1).any(), st
    for k in rows:
        assert bool(torch.isnan(out[k][1]).any()), k
        assert bool(torch.isfinite(out[k][[0, 2]]).all()), k


# ---- tfmpc_tvlqr_{solve,backward,forward}_f32 / _f64 -------------------------------------------------------------------

TV_SHAPES = [(F32, 16, 8, 5, "tv_mfma_16x8"), (F32, 3, 2, 5, "tv_mfma_16x8 (zero-padded)"), (F32, 20, 10, 5, "tv_generic_wave"),
             (F32, 49, 16, 5, "tv_generic_wave"), (F32, 16, 8, 53, "tv_mfma_16x8"),      # T = 53: the model ring has wrapped
             (F64, 12, 5, 5, "tv_f64_wave16"), (F64, 16, 8, 5, "tv_f64_wave16"), (F64, 20, 10, 5, "tv_f64_wave32"),
             (F64, 32, 32, 5, "tv_f64_wave32")]
_ids = lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None      # noqa: E731


def _tv_workspace_bytes(dtype, B, n, m, T):
    query = _lib().tfmpc_tvlqr_workspace_bytes_f64 if dtype == F64 else _lib().tfmpc_tvlqr_workspace_bytes
    return int(query(B, n, m, T))


@pytest.mark.parametrize("flagged", [False, True], ids=["clean", "flagged"])
@pytest.mark.parametrize("dtype,n,m,T,kernel", TV_SHAPES, ids=_ids)
def test_tvlqr_solve(dtype, n, m, T, kernel, flagged):
    assert _name("tfmpc_tvlqr_kernel_name_f64" if dtype == F64 else "tfmpc_tvlqr_kernel_name", n, m, T) == kernel
    B = 3
    tv, x0, _ = _tv(_problem(n, m, T, B, dtype, flagged=flagged), dtype)
    fields = ("states", "actions", "costs", "status", "K", "k", "V", "v", "const")
    options = [dict(), dict(want_policy=True), dict(want_value=True), dict(want_policy=True, want_value=True)]
    if dtype == F64:
        options.append(dict(want_v=True))
    ws_bytes = _tv_workspace_bytes(dtype, B, n, m, T)
    assert ws_bytes > 0
    for opt in options:
        def call(workspace=None, opt=opt):
            out = tv.solve_device(x0, workspace=workspace, **opt)
            assert tv.last_status is out["status"] and (workspace is None or out["workspace"] is workspace)
            tensors = {k: out[k] for k in fields if k in out}
            return tensors, tuple(tensors)

        scratch = not opt.get("want_policy")                 # the gains live in the workspace
        first = _run(call, ws_bytes if scratch else 0, what=opt)
        assert ("K" in first) == bool(opt.get("want_policy")) and ("V" in first) == bool(opt.get("want_value"))
        _expect_flag(first, flagged, rows=())                # (the plain solve flags the instance in its status only)
        if scratch:                                          # one caller-owned workspace, pre-filled in place
            ws = torch.empty(ws_bytes // x0.element_size() + 1, dtype=dtype, device="cuda")
            for i, pattern in enumerate(PATTERNS):
                fill(ws, pattern, seed=i)
                with StaleMemory(pattern, seed=i) as mem:
                    tensors, made = call(ws)
                    torch.cuda.synchronize()
                mem.check({k: tensors[k] for k in made})
                for k in first:
                    assert same(first[k], tensors[k]), (opt, k, pattern, "caller-owned workspace")

    def split():                                             # backward, then forward: no workspace, five plus three outputs
        policy, value = tv.backward()
        states, actions, costs = tv.forward(policy, x0)
        tensors = dict(K=policy.K, k=policy.k, V=value.V, v=value.v, const=value.const, states=states, actions=actions,
                       costs=costs, status=tv.last_status)
        return tensors, tuple(k for k in tensors if k != "status")

    both = _run(split, what="split")
    _expect_flag(both, flagged, rows=())


# ---- tfmpc_tvlqr_solve_time_parallel_f64 -------------------------------------------------------------------------------

TP_CASES = [(16, 8, 23, 4, "tv_f64_time_parallel16"),       # a ragged last segment
            (20, 10, 9, 9, "tv_f64_time_parallel32"),       # one step per segment
            (5, 3, 7, 5, "tv_f64_time_parallel16"),         # ceil(7 / 2) = 4 segments, not the five asked for
            (17, 8, 1, 5, "tv_f64_wave32")]                 # forwards to the sequential kernel


@pytest.mark.parametrize("final", [None, "per"], ids=["default", "final"])
@pytest.mark.parametrize("flagged", [False, True], ids=["clean", "flagged"])
@pytest.mark.parametrize("n,m,T,segments,kernel", TP_CASES)
def test_time_parallel_solve(n, m, T, segments, kernel, flagged, final):
    assert _name("tfmpc_tvlqr_time_parallel_kernel_name_f64", n, m, T, segments) == kernel
    if (n, m, T) == (5, 3, 7):
        assert len(tp.segment_table(T, segments)[1]) == 4
    B = 3
    tv, x0, _ = _tv(_problem(n, m, T, B, F64, final=final, flagged=flagged), F64)     # (flagged: step T // 2, a middle segment)
    ws_bytes = int(_lib().tfmpc_tvlqr_time_parallel_workspace_bytes_f64(B, n, m, T, segments))
    assert ws_bytes > 0
    fields = ("states", "actions", "costs", "status", "K", "k", "V", "v")
    for want_policy, want_value in ((False, False), (True, False), (False, True), (True, True)):
        def call(want_policy=want_policy, want_value=want_value):
            out = tv._time_parallel_device(x0, segments, want_policy, want_value)
            tensors = {k: out[k] for k in fields if k in out}
            return tensors, tuple(tensors)

        first = _run(call, ws_bytes, what=(want_policy, want_value))
        assert ("K" in first) == want_policy and ("V" in first) == want_value
        # the finish kernel gives a flagged instance NaN rows; one segment is the sequential solve: status only
        _expect_flag(first, flagged, rows=("states", "actions", "costs") if "time_parallel" in kernel else ())


# ---- tfmpc_tvlqr_vjp_f32 / _f64 through solve_tensors(differentiable=True), what tvlqr_solve calls ----------------------

def _weights(B, T, n, m, loss, dtype, seed=3):
    rng = np.random.default_rng(seed)
    w = (rng.normal(size=(B, T + 1, n, 1)), rng.normal(size=(B, T, m, 1)), rng.normal(size=(B, T + 1, 1, 1)))
    return tuple(_dev(g, dtype) if loss in (name, "mixed") else None for g, name in zip(w, LOSSES))


def _weighted(outs, w):
    return sum((out * g).sum() for out, g in zip(outs, w) if g is not None)


def _vjp_workspace_bytes(dtype, B, n, m, T):
    query = _lib().tfmpc_tvlqr_vjp_workspace_bytes_f64 if dtype == F64 else _lib().tfmpc_tvlqr_vjp_workspace_bytes
    return max(int(query(B, n, m, T)), _tv_workspace_bytes(dtype, B, n, m, T))


SHARING = dict(per=dict(), batch=dict(shared=MODEL), time=dict(const=("F", "f", "C")), both=dict(shared=MODEL, const=("F", "C", "c")),
               x0=dict(shared=("C", "c"), const=("f", "C"), x0_shared=True), Ff=dict(shared=("F", "f")))
# (sharing, final cost, loss, B, flagged): every sharing, final-cost form and loss once; the second chunk of one instance
# under both reductions (per step and per instance); a flagged instance per instance and inside a batch sum
GRAD_CONFIGS = [("per", None, "mixed", 3, False), ("batch", "shared", "states", 3, False), ("time", "per", "actions", 3, False),
                ("both", None, "costs", 3, False), ("x0", "shared", "mixed", 3, False), ("batch", "per", "costs", 3, False),
                ("batch", "shared", "mixed", 257, False), ("both", None, "costs", 257, False), ("x0", None, "actions", 257, False),
                ("per", "per", "mixed", 3, True), ("Ff", None, "mixed", 3, True)]
# (16, 8): reductions on the matrix cores (n <= 16 and d <= 32); (17, 2), (20, 10): generic; (16, 17): d = 33
GRAD_SHAPES = [(16, 8, "tv_mfma_16x8", "tv_f64_wave16"), (17, 2, "tv_generic_wave", "tv_f64_wave32"),
               (20, 10, "tv_generic_wave", "tv_f64_wave32"), (16, 17, "tv_generic_wave", "tv_f64_wave32")]


def _solve_gradients(n, m, T, B, dtype, sharing, final, loss, flagged):
    ops = _problem(n, m, T, B, dtype, final=final, flagged=flagged, seed=5, **SHARING[sharing])
    w = _weights(B, T, n, m, loss, dtype)
    ws_bytes = _vjp_workspace_bytes(dtype, B, n, m, T)
    assert ws_bytes > 0

    def call():
        tv, x0, leaves = _tv(ops, dtype, leaves=True)
        outs = tv.solve_tensors(x0, differentiable=True)
        assert outs[0].requires_grad and outs[0].shape == (B, T + 1, n, 1)
        names = [k for k, v in leaves.items() if v is not None]
        grads = torch.autograd.grad(_weighted(outs, w), [leaves[k] for k in names])
        tensors = dict(states=outs[0], actions=outs[1], costs=outs[2], status=tv.last_status, grad_status=tv.last_grad_status)
        tensors.update({"d" + k: g for k, g in zip(names, grads)})
        return tensors, tuple(k for k in tensors if k != "grad_status")     # (grad_status: torch.zeros)

    first = _run(call, ws_bytes, what=(sharing, final, loss, B, flagged))
    for k, v in ops.items():
        assert first["d" + k].shape[:v.ndim] == v.shape, k                    # each gradient in its operand's shape
    if flagged:
        _expect_flag(first, True, status="grad_status", rows=())
        summed = SHARING[sharing].get("shared", ())
        for k in ops:
            g = first["d" + k]
            if k in summed:
                assert bool(torch.isnan(g).all()), k                          # a sum that contains the flagged instance
            else:
                assert bool(torch.isnan(g[1]).all()) and bool(torch.isfinite(g[[0, 2]]).all()), k
    else:
        assert not first["grad_status"].any()
        for k in ops:
            assert bool(torch.isfinite(first["d" + k]).all()), k
    return first


@pytest.mark.parametrize("sharing,final,loss,B,flagged", GRAD_CONFIGS)
@pytest.mark.parametrize("n,m,kernel32,kernel64", GRAD_SHAPES)
@pytest.mark.parametrize("dtype", [F32, F64], ids=_ids)
def test_tvlqr_solve_gradients(dtype, n, m, kernel32, kernel64, sharing, final, loss, B, flagged):
    T = 5
    assert _name("tfmpc_tvlqr_kernel_name", n, m, T) == kernel32 and _name("tfmpc_tvlqr_kernel_name_f64", n, m, T) == kernel64
    _solve_gradients(n, m, T, B, dtype, sharing, final, loss, flagged)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("sharing", ["per", "batch", "time", "both"])
@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=_ids)
def test_tvlqr_solve_gradients_every_loss_under_every_sharing(dtype, n, m, sharing, loss):
    """The losses decide gx, gu, gc and with them which branches of the fold run, the sharing which records the sweep stores."""
    _solve_gradients(n, m, 5, 3, dtype, sharing, None, loss, False)


# ---- tfmpc_tvlqr_backward_vjp_f32 through backward(differentiable=True), what tvlqr_backward calls ---------------------

BACKWARD_SHAPES = [(16, 8, "tvb_vjp_mfma_16"), (20, 10, "tvb_vjp_mfma_32")]
UPSTREAM = dict(gK=("gK",), value0=("gV", "gv", "gconst"), all=None)


# (the recursion's batch axis comes from its operands alone: c keeps it where the others are shared)
BACKWARD_SHARING = dict(per=dict(), batch=dict(shared=("F", "f", "C")), both=dict(shared=("F", "f", "C"), const=("F", "C", "c")))
BACKWARD_CONFIGS = [(B, *cfg) for B in (1, 3, 257) for cfg in (("per", "per", False), ("batch", "shared", False), ("both", None, False))]
BACKWARD_CONFIGS.append((3, "per", None, True))


@pytest.mark.parametrize("B,sharing,final,flagged", BACKWARD_CONFIGS)
@pytest.mark.parametrize("subset", list(UPSTREAM))
@pytest.mark.parametrize("n,m,kernel", BACKWARD_SHAPES)
def test_tvlqr_backward_gradients(n, m, kernel, B, subset, sharing, final, flagged):
    T = 5
    assert _name("tfmpc_tvlqr_backward_vjp_kernel_name", n, m, T) == kernel
    ws_bytes = int(_lib().tfmpc_tvlqr_backward_vjp_workspace_bytes(B, n, m, T))
    assert (ws_bytes == 0) == (B == 1)                             # B = 1: no reduction, no scratch
    ops = _problem(n, m, T, B, F32, final=final, flagged=flagged, seed=9, **BACKWARD_SHARING[sharing])
    ops.pop("x0")
    up = bwref.upstream(n, m, T, B, seed=4, only=UPSTREAM[subset])
    if subset == "value0":
        for name in UPSTREAM[subset]:
            up[name][:, 1:] = 0.0
    up = [_dev(up[name], F32) for name in bwref.UPS]
    if B > 3:                                                      # keep a summed gradient's size that of a small batch's
        up = [None if g is None else g / B for g in up]

    def call():
        tv, _, leaves = _tv(dict(ops, x0=np.zeros((B, n), np.float32)), F32, leaves=True)
        policy, value = tv.backward(differentiable=True)
        outs = (policy.K, policy.k, value.V, value.v, value.const)
        total = sum((out * g.reshape(out.shape)).sum() for out, g in zip(outs, up) if g is not None)
        names = [k for k, v in leaves.items() if v is not None and k != "x0"]
        grads = torch.autograd.grad(total, [leaves[k] for k in names])
        tensors = dict(zip(("K", "k", "V", "v", "const"), outs), status=tv.last_status, grad_status=tv.last_grad_status)
        tensors.update({"d" + k: g for k, g in zip(names, grads)})
        return tensors, tuple(k for k in tensors if k not in ("status", "grad_status"))

    first = _run(call, ws_bytes, what=(B, subset, sharing, final, flagged))
    if flagged:
        _expect_flag(first, True, status="grad_status", rows=("dF", "dC"))
    else:
        assert not first["grad_status"].any() and all(bool(torch.isfinite(v).all()) for v in first.values())


@pytest.mark.parametrize("n,m,kernel", BACKWARD_SHAPES)
def test_tvlqr_backward_all_upstream_null_gives_exact_zeros_under_every_fill(n, m, kernel):
    """The C ABI call of test_all_upstream_null_gives_exact_zeros with outputs and workspace from ``torch.empty``: the
    exact-zero gradients are zeros whatever the buffers held."""
    from test_tvlqr_backward_grad_gpu import _abi_call
    T, B, d = 5, 3, n + m
    assert _name("tfmpc_tvlqr_backward_vjp_kernel_name", n, m, T) == kernel
    tv, _, _ = _tv(_problem(n, m, T, B, F32, seed=9), F32)
    policy, value = tv.backward()
    fwd = [policy.K, policy.k, value.V, value.v, tv.last_status]
    ws_bytes = int(_lib().tfmpc_tvlqr_backward_vjp_workspace_bytes(B, n, m, T))
    assert ws_bytes > 0

    def call():
        outs = [torch.empty((B, T, size), device="cuda") for size in (n * d, n, d * d, d)]
        ws = torch.empty(ws_bytes // 4 + 1, device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        assert _abi_call(_lib(), B, n, m, T, [tv.F, tv.f, tv.C, tv.c], fwd, [None] * 5, outs, status, ws) == 0
        return dict(zip(("dF", "df", "dC", "dc"), outs), status=status), ("dF", "df", "dC", "dc")

    first = _run(call, ws_bytes)
    for k, v in first.items():
        assert not v.any(), k


# ---- tfmpc_tvlqr_box_solve_f32 / _f64 ----------------------------------------------------------------------------------

BOX_SHAPES = [(16, 8, 5, "tv_box_wave", "tv_box_f64_wave16"), (5, 3, 5, "tv_box_wave", "tv_box_f64_wave16"),
              (32, 32, 4, "tv_box_wave", "tv_box_f64_wave32"), (5, 3, 1, "tv_box_wave", "tv_box_f64_wave16")]
BOX_FIELDS = ("states", "actions", "costs")


def _bounds(n, m, T, B, form="BTm", held="some"):
    """``lqr_box_grad_ref.tv_bounds`` rounded to fp32 numbers, in the form the caller passes: scalar, [m], [T, m], [B, 1, m]
    or [B, T, m]; ``held``: "some", "all" (a pinned box, low == high) or "none" (+-inf)."""
    low, high = (a.astype(np.float32).astype(np.float64) for a in bref.tv_bounds(n, m, T, B))
    if held == "none":
        low, high = np.full_like(low, -INF), np.full_like(high, INF)
    elif held == "all":
        high = low
    pick = {"scalar": lambda a: a[0, 0, 0], "m": lambda a: a[0, 0], "Tm": lambda a: a[0], "B1m": lambda a: a[:, :1], "BTm": lambda a: a}
    return np.array(pick[form](low)), np.array(pick[form](high))


def _box_call(t, dtype, **kw):
    res = tvlqr_box_solve(t["F"], t["f"], t["C"], t["c"], t["x0"], t["low"], t["high"], C_final=t.get("Cfin"),
                          c_final=t.get("cfin"), dtype=dtype, **kw)
    info = res.info
    tensors = dict(zip(BOX_FIELDS, res), status=info.last_status, iterations=info.last_iterations, reason=info.last_reason,
                   clamped=info.last_clamped)
    return tensors, BOX_FIELDS                                      # (status, iterations, reason, mask: torch.zeros)


def _box_workspace_bytes(dtype, B, n, m, T):
    query = _lib().tfmpc_tvlqr_box_solve_workspace_bytes_f64 if dtype == F64 else _lib().tfmpc_tvlqr_box_solve_workspace_bytes
    return int(query(B, n, m, T))


@pytest.mark.parametrize("n,m,T,kernel32,kernel64", BOX_SHAPES)
@pytest.mark.parametrize("dtype", [F32, F64], ids=_ids)
def test_tvlqr_box_solve(dtype, n, m, T, kernel32, kernel64):
    assert _name("tfmpc_tvlqr_box_solve_kernel_name", n, m, T) == kernel32
    assert _name("tfmpc_tvlqr_box_solve_kernel_name_f64", n, m, T) == kernel64
    B = 3
    ws_bytes = _box_workspace_bytes(dtype, B, n, m, T)
    assert ws_bytes > 0
    ops = _problem(n, m, T, B, dtype, final="per", seed=13)

    def tensors_of(held="some", form="BTm", flagged=False):
        o = _problem(n, m, T, B, dtype, final="per", seed=13, flagged=True) if flagged else ops
        low, high = _bounds(n, m, T, B, form, held)
        return {k: _dev(v, dtype) for k, v in dict(o, low=low, high=high).items()}

    t = tensors_of()
    base = _run(lambda: _box_call(t, dtype), ws_bytes, what="bounded")
    assert not base["status"].any() and not base["reason"].any() and bool(base["clamped"].any())
    # ... a warm start at the rounded optimum: converged in the first sweep
    warm = _run(lambda: _box_call(t, dtype, u_init=base["actions"][..., 0]), ws_bytes, what="warm start")
    assert not warm["status"].any() and not warm["reason"].any()
    assert int(warm["iterations"].max()) <= max(2, int(base["iterations"].max()))
    # ... the pass cap
    capped = _run(lambda: _box_call(t, dtype, max_iter=1), ws_bytes, what="max_iter = 1")
    assert int(capped["iterations"].max()) <= 1
    # ... without bounds, in every other form the bounds come in
    t = tensors_of(held="none", form="scalar")
    free = _run(lambda: _box_call(t, dtype), ws_bytes, what="no bounds")
    assert not free["status"].any() and not free["clamped"].any()
    for form in ("m", "Tm", "B1m"):
        t = tensors_of(form=form)
        out = _run(lambda: _box_call(t, dtype), ws_bytes, what=form)
        assert not out["status"].any()
    # ... a pinned box: the zero-sweep exit
    t = tensors_of(held="all")
    pinned = _run(lambda: _box_call(t, dtype), ws_bytes, what="pinned")
    assert not pinned["iterations"].any() and not pinned["status"].any() and not pinned["reason"].any()
    assert torch.equal(pinned["actions"][..., 0], t["low"])
    # ... a flagged instance
    if T > 1:
        t = tensors_of(flagged=True)
        bad = _run(lambda: _box_call(t, dtype), ws_bytes, what="flagged")
        _expect_flag(bad, True)
        assert int(bad["reason"][1]) == 3


# ---- tfmpc_tvlqr_box_vjp_f32 / _f64 ------------------------------------------------------------------------------------

BOX_VJP_SHAPES = [(16, 8, "tv_masked_16x8", "tv_masked_f64_wave16"), (5, 3, "tv_masked_16x8 (zero-padded)", "tv_masked_f64_wave16"),
                  (20, 10, "tv_masked_generic_wave", "tv_masked_f64_wave32"), (8, 32, "tv_masked_generic_wave", "tv_masked_f64_wave32")]
# (sharing, final, bounds' form, held, loss, B, flagged)
BOX_VJP_CONFIGS = [("per", None, "BTm", "some", "mixed", 3, False), ("per", "per", "BTm", "some", "states", 3, False),
                   ("per", None, "BTm", "some", "actions", 3, False),           # a loss without a cost term: the exact zeros
                   ("batch", "shared", "scalar", "some", "mixed", 3, False), ("time", None, "m", "some", "costs", 3, False),
                   ("both", None, "Tm", "some", "mixed", 3, False), ("per", None, "B1m", "some", "mixed", 3, False),
                   ("per", None, "scalar", "none", "mixed", 3, False), ("per", None, "BTm", "all", "mixed", 3, False),
                   ("batch", None, "Tm", "some", "mixed", 257, False),          # the Rlo / Rhi reductions, a second chunk of one
                   ("batch", "shared", "m", "some", "actions", 257, False),
                   ("per", None, "BTm", "some", "mixed", 3, True), ("time", None, "Tm", "some", "mixed", 3, True)]


def _box_vjp_workspace_bytes(dtype, B, n, m, T):
    query = _lib().tfmpc_tvlqr_box_vjp_workspace_bytes_f64 if dtype == F64 else _lib().tfmpc_tvlqr_box_vjp_workspace_bytes
    return int(query(B, n, m, T))


def _box_problem(n, m, T, B, dtype, sharing, final, form, held, flagged):
    """-> (tensors by name, states, actions of the forward on the clean problem).  ``flagged``: instance 1's R block is
    -1e3 I at the step where most of its controls are free, so the masked adjoint meets it; its trajectory stays that of
    its clean twin."""
    kw = {k: v for k, v in SHARING[sharing].items() if k != "x0_shared"}
    low, high = _bounds(n, m, T, B, form, held)
    t = {k: _dev(v, dtype) for k, v in dict(_problem(n, m, T, B, dtype, final=final, seed=21, **kw), low=low, high=high).items()}
    res = tvlqr_box_solve(t["F"], t["f"], t["C"], t["c"], t["x0"], t["low"], t["high"], C_final=t.get("Cfin"),
                          c_final=t.get("cfin"), dtype=dtype)
    torch.cuda.synchronize()
    assert not res.info.last_status.any()
    states, actions = res[0][..., 0].detach().clone(), res[1][..., 0].detach().clone()
    if flagged:
        free = (actions != torch.broadcast_to(t["low"], actions.shape)) & (actions != torch.broadcast_to(t["high"], actions.shape))
        assert bool(free[1].any())
        step = 0 if t["C"].shape[1] == 1 else int(free[1].sum(-1).argmax())
        t["C"] = t["C"].clone()
        t["C"][1, step, n:, n:] = -1.0e3 * torch.eye(m, device="cuda", dtype=dtype)
    return t, states, actions


@pytest.mark.parametrize("sharing,final,form,held,loss,B,flagged", BOX_VJP_CONFIGS)
@pytest.mark.parametrize("n,m,kernel32,kernel64", BOX_VJP_SHAPES)
@pytest.mark.parametrize("dtype", [F32, F64], ids=_ids)
def test_tvlqr_box_vjp(dtype, n, m, kernel32, kernel64, sharing, final, form, held, loss, B, flagged):
    T = 5
    assert _name("tfmpc_tvlqr_box_vjp_kernel_name", n, m, T) == kernel32
    assert _name("tfmpc_tvlqr_box_vjp_kernel_name_f64", n, m, T) == kernel64
    t, states, actions = _box_problem(n, m, T, B, dtype, sharing, final, form, held, flagged)
    w = _weights(B, T, n, m, loss, dtype)
    ws_bytes = _box_vjp_workspace_bytes(dtype, B, n, m, T)
    assert ws_bytes > 0

    def call():
        got = tvlqr_box_vjp(t["F"], t["f"], t["C"], t["c"], t["low"], t["high"], states, actions, *w, C_final=t.get("Cfin"),
                            c_final=t.get("cfin"), dtype=dtype)
        return dict(got), tuple(k for k in got if k not in ("clamped", "status"))      # (mask, status: torch.zeros)

    first = _run(call, ws_bytes, what=(sharing, final, form, held, loss, B, flagged))
    assert set(first) >= {"F", "f", "C", "c", "x0", "low", "high", "clamped", "status"}
    clamped = first["clamped"]
    assert {"some": bool(clamped.any()) and not bool(clamped.all()), "all": bool(clamped.all()), "none": not bool(clamped.any())}[held]
    if flagged:
        st = first["status"].cpu().numpy()
        assert st[1] != 0 and not np.delete(st, 1).any(), st
        assert bool(torch.isnan(first["x0"][1]).all()) and bool(torch.isfinite(first["x0"][[0, 2]]).all())
    else:
        assert not first["status"].any()
        assert all(bool(torch.isfinite(v).all()) for k, v in first.items() if v.is_floating_point()), first.keys()
        if form == "BTm" and sharing == "per" and loss in ("states", "actions"):
            # a loss without a cost term: the bounds' gradients off the held set and dc of a held control are exact zeros
            assert not first["low"][~clamped].any() and not first["high"][~clamped].any()
            assert not first["c"][..., n:][clamped].any()


@pytest.mark.parametrize("loss", ["mixed", "states"])
@pytest.mark.parametrize("n,m", [(16, 8), (5, 3), (20, 10), (8, 32)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=_ids)
def test_tvlqr_box_solve_differentiable(dtype, n, m, loss):
    """Forward and backward of one call under the same fill: every operand per instance and per step, so that each leaf's
    gradient is the buffer tvlqr_box_vjp allocated."""
    T, B = 5, 3
    low, high = _bounds(n, m, T, B)
    ops = dict(_problem(n, m, T, B, dtype, final="per", seed=21), low=low, high=high)
    w = _weights(B, T, n, m, loss, dtype)
    ws_bytes = max(_box_vjp_workspace_bytes(dtype, B, n, m, T), _box_workspace_bytes(dtype, B, n, m, T))

    def call():
        leaves = {k: _dev(v, dtype).requires_grad_() for k, v in ops.items()}
        res = tvlqr_box_solve(leaves["F"], leaves["f"], leaves["C"], leaves["c"], leaves["x0"], leaves["low"], leaves["high"],
                              C_final=leaves["Cfin"], c_final=leaves["cfin"], dtype=dtype, differentiable=True)
        grads = torch.autograd.grad(_weighted(res, w), list(leaves.values()))
        info = res.info
        tensors = dict(zip(BOX_FIELDS, res), status=info.last_status, iterations=info.last_iterations, reason=info.last_reason,
                       clamped=info.last_clamped, grad_status=info.last_grad_status)
        tensors.update({"d" + k: g for k, g in zip(leaves, grads)})
        return tensors, BOX_FIELDS + tuple("d" + k for k in leaves)

    first = _run(call, ws_bytes, what=loss)
    assert not first["status"].any() and not first["grad_status"].any() and bool(first["clamped"].any())
    assert all(bool(torch.isfinite(first["d" + k]).all()) for k in ops)


# ---- tfmpc_lqr_steady_state_f32 / _f64, tfmpc_lqr_steady_state_vjp_f32 -------------------------------------------------

SS_SHAPES = [(1, 1, "ss_mfma_16 (padded)", "ss_f64_wave16", "ss_vjp_mfma_16 (padded)"), (16, 8, "ss_mfma_16", "ss_f64_wave16", "ss_vjp_mfma_16"),
             (20, 10, "ss_wave_32", "ss_f64_wave32", "ss_vjp_wave_32")]
ST_NOT_STABILISING = _hip.ST_NOT_STABILISING


def _ss_operands(n, m, B, unstable):
    F, f, C, c = ssref.make_lqr_batch(n, m, B, seed=41 + n)
    if unstable:                                                   # instance 1: an unstable mode no input reaches
        F, C = F.copy(), C.copy()
        F[1, 0, :] = 0.0
        F[1, :, 0] = 0.0
        F[1, 0, 0] = 1.5
        C[1, 0, 1:] = 0.0
        C[1, 1:, 0] = 0.0
    return dict(F=F, f=f, C=C, c=c)


@pytest.mark.parametrize("shared,unstable", [((), False), ((), True), (("F", "C"), False), (MODEL, False)],
                         ids=["per", "not-stabilising", "shared-F-C", "unbatched"])
@pytest.mark.parametrize("n,m,kernel32,kernel64,kernel_vjp", SS_SHAPES)
def test_steady_state_and_its_gradients(n, m, kernel32, kernel64, kernel_vjp, shared, unstable):
    assert _name("tfmpc_lqr_steady_state_kernel_name", n, m) == kernel32
    assert _name("tfmpc_lqr_steady_state_kernel_name_f64", n, m) == kernel64
    assert _name("tfmpc_lqr_steady_state_vjp_kernel_name", n, m) == kernel_vjp
    B = 3
    unbatched = shared == MODEL
    ops = {k: (v[0] if k in shared else v) for k, v in _ss_operands(n, m, B, unstable).items()}
    rng = np.random.default_rng(6)
    keep = torch.ones(1 if unbatched else B, device="cuda")
    if unstable:
        keep[1] = 0.0
    ws_bytes = int(_lib().tfmpc_lqr_steady_state_vjp_workspace_bytes(B, n, m)) if shared and not unbatched else 0
    weights = None

    def call():
        nonlocal weights
        leaves = {k: _dev(v, F32).requires_grad_() for k, v in ops.items()}
        lqr = LQR(*leaves.values(), device="cuda")
        ss = lqr.steady_state(differentiable=True)
        outs = dict(K=ss.K, k=ss.k, P=ss.P, p=ss.p)
        if weights is None:
            weights = {k: _dev(rng.normal(size=tuple(v.shape)), F32) for k, v in outs.items()}
        mask = keep if not unbatched else keep[0]
        total = sum((torch.nan_to_num(v, nan=0.0) * weights[k] * (mask.reshape(-1, 1, 1) if not unbatched else mask)).sum()
                    for k, v in outs.items())
        grads = torch.autograd.grad(total, list(leaves.values()))
        tensors = dict(outs, iterations=ss.iterations, status=ss.status, grad_status=lqr.last_grad_status)
        tensors.update({"d" + k: g for k, g in zip(leaves, grads)})
        return tensors, ("K", "k", "P", "p") + tuple("d" + k for k in leaves)

    first = _run(call, ws_bytes, what=(shared, unstable))
    if unstable:
        st = first["grad_status"].cpu().numpy()
        assert st[1] & ST_NOT_STABILISING and not st[[0, 2]].any() and int(first["status"][1]) & ST_NOT_STABILISING, st
        for k in ("K", "P", "dF", "dC"):
            assert bool(torch.isnan(first[k][1]).all()) and bool(torch.isfinite(first[k][[0, 2]]).all()), k
    else:
        assert not first["status"].any() and not first["grad_status"].any()
        assert all(bool(torch.isfinite(v).all()) for v in first.values())

    def double():                                                  # the double forward of the same numbers
        ss = lqr_steady_state(*(_dev(v, F64) for v in ops.values()), dtype=F64)
        return dict(K=ss.K, k=ss.k, P=ss.P, p=ss.p, iterations=ss.iterations, status=ss.status), ("K", "k", "P", "p")

    first = _run(double, what=("f64", shared, unstable))
    st = first["status"].reshape(-1).cpu().numpy()
    assert (st[1] & ST_NOT_STABILISING and not st[[0, 2]].any()) if unstable else not st.any(), st


# ---- streams -----------------------------------------------------------------------------------------------------------

def test_concurrent_streams_do_not_interfere_multi_launch_families():
    """After test_workspace_independence_gpu.py::test_concurrent_streams_do_not_interfere, for families that enqueue 4 to
    12 launches per call: a double VJP, a time-parallel solve and a box solve in flight on three streams for three rounds,
    each call allocating inside its stream context (under the garbage fill), return the bits of the same calls run one
    after the other."""
    B, T = 64, 20
    vjp_ops = _problem(16, 8, T, B, F64, final="shared", seed=31, shared=("F", "C"))
    w = _weights(B, T, 16, 8, "mixed", F64)
    tv_tp, x0_tp, _ = _tv(_problem(20, 10, 40, 8, F64, seed=32), F64)
    low, high = _bounds(16, 8, T, B)
    box = {k: _dev(v, F32) for k, v in dict(_problem(16, 8, T, B, F32, seed=33), low=low, high=high).items()}

    def vjp_job():
        tv, x0, leaves = _tv(vjp_ops, F64, leaves=True)
        outs = tv.solve_tensors(x0, differentiable=True)
        names = [k for k, v in leaves.items() if v is not None]
        grads = torch.autograd.grad(_weighted(outs, w), [leaves[k] for k in names])
        return dict({"d" + k: g for k, g in zip(names, grads)}, states=outs[0], costs=outs[2], grad_status=tv.last_grad_status)

    def tp_job():
        out = tv_tp._time_parallel_device(x0_tp, 6, True, True)
        return {k: out[k] for k in ("states", "actions", "costs", "status", "K", "k", "V", "v")}

    def box_job():
        return _box_call(box, F32)[0]

    jobs = [vjp_job, tp_job, box_job]
    serial = []
    for job in jobs:
        out = job()
        torch.cuda.synchronize()
        serial.append(_snapshot(out))
    assert not serial[0]["grad_status"].any() and not serial[1]["status"].any() and not serial[2]["status"].any()
    streams = [torch.cuda.Stream() for _ in jobs]
    outs = [None] * len(jobs)
    torch.cuda.synchronize()
    with StaleMemory("garbage", seed=5) as mem:
        for rep in range(3):
            for i, (job, st) in enumerate(zip(jobs, streams)):
                with torch.cuda.stream(st):
                    outs[i] = job()
        torch.cuda.synchronize()
    mem.check(workspace_bytes=int(_lib().tfmpc_tvlqr_vjp_workspace_bytes_f64(B, 16, 8, T)))
    for ref, out in zip(serial, outs):
        for k in ref:
            assert same(ref[k], out[k]), k
