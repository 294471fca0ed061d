"""Double-precision gradients of the finite-horizon Riccati recursion on the MI355X:
``tvlqr_backward(..., dtype=torch.float64)`` (tfmpc_tvlqr_backward_f64 forward, tfmpc_tvlqr_backward_vjp_f64 backward) and
``tvlqr_backward_vjp`` against the 80-bit closed form of tests/tvlqr_backward_grad_f64_ref.py under its budget rule
(tests/test_tvlqr_backward_grad_f64_cpu.py shows on the host that the rule is attainable on these inputs), the summed
gradients bit for bit against the stated orders, bit stability, status isolation, the unchanged forward and fp32 bits,
``gradcheck``, a value loss over many x0, the gain over the fp32 path and stale memory.

Every case prints its measured ratios; with TFMPC_ACCURACY_OUT=<file> the budget cases' ratios are written there as JSON
(profiles/tvlqr_backward_grad_f64_accuracy.json is such a file)."""

import json
import os

import numpy as np
import pytest
import torch

import batch_sum_f64_ref as sum64
import tvlqr_backward_grad_f64_ref as g64
import tvlqr_backward_grad_ref as gref
import tvlqr_f64_ref as ref64
from stale_memory import PATTERNS, StaleMemory, same
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR, tvlqr_backward, tvlqr_backward_vjp

pytestmark = pytest.mark.gpu

OPS = ("F", "f", "C", "c", "Cfin", "cfin")
GRAD_OF = dict(F="dF", f="df", C="dC", c="dc", Cfin="dCfin", cfin="dcfin")
OUTS = ("K", "k", "V", "v", "const")
ST_NOT_PD = gref.ST_NOT_PD
F64 = torch.float64
_MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _accuracy_file():
    yield
    path = os.environ.get("TFMPC_ACCURACY_OUT")
    if path and _MEASURED:
        with open(path, "w") as out:
            json.dump({"rule": "error vs 80-bit closed form / max(fp64 closed form, fp64 autograd, fp64 closed form from the "
                               "kernel's forward, 2^-48 scale): [median, max] over instances", "cases": _MEASURED}, out, indent=1)
            out.write("\n")


def _name(n, m, T=5):
    return _hip.load().tfmpc_tvlqr_backward_vjp_kernel_name_f64(n, m, T).decode()


def _problem(n, m, T, B=4, seed=None, final=False, unscaled=False, only=None):
    """Operands as float64 numpy (a dict over OPS) and the upstream gradients (a dict over UPS)."""
    seed = 100 * n + m if seed is None else seed
    if unscaled:
        F, f, C, c = ref64.make_unscaled(n, m, T, B, seed=seed)
        Cf = cf = None
    else:
        F, f, C, c, Cf, cf = gref.problem(n, m, T, B, seed=seed, final=final)
    ops = dict(zip(OPS, g64.as_f64(F, f, C, c, Cf, cf)))
    ups = {k: (None if v is None else v.astype(np.float64)) for k, v in gref.upstream(n, m, T, B, seed=seed, only=only).items()}
    return ops, ups


def _leaves(ops):
    return {name: (None if a is None else torch.as_tensor(a, device="cuda", dtype=F64).requires_grad_()) for name, a in ops.items()}


def _loss(outs, ups):
    total = 0
    for out, g in zip(outs, (ups[name] for name in g64.UPS)):
        if g is not None:
            total = total + (out * torch.as_tensor(g, device=out.device).reshape(out.shape)).sum()
    return total


def _host_fwd(outs):
    fwd = {name: o.detach().cpu().numpy() for name, o in zip(OUTS, outs)}
    B, T, m, n = fwd["K"].shape
    fwd.update(k=fwd["k"].reshape(B, T, m), v=fwd["v"].reshape(B, T, n))
    return fwd


def _autograd(ops, ups):
    """Through ``tvlqr_backward(dtype=torch.float64)``: (gradients by GRADS name as numpy, the kernel's forward outputs)."""
    leaves = _leaves(ops)
    outs = tvlqr_backward(*(leaves[name] for name in OPS), dtype=F64)
    assert all(o.dtype == F64 for o in outs)
    _loss(outs, ups).backward()
    torch.cuda.synchronize()
    got = {GRAD_OF[name]: t.grad.cpu().numpy() for name, t in leaves.items() if t is not None}
    assert all(t.grad.dtype == F64 and t.grad.shape == t.shape for t in leaves.values() if t is not None)
    return got, _host_fwd(outs)


def _forward(ops):
    """The double recursion of ``ops``: (K, k, V, v, const) batched cuda tensors and its status."""
    tv = TimeVaryingLQR(*(ops[name] for name in OPS), device="cuda", dtype=F64)
    outs = tv._backward_launch()
    return outs[:5], outs[5]


def _vjp(ops, fwd, status, ups):
    """``tvlqr_backward_vjp``: (gradients by GRADS name as cuda tensors, the returned status)."""
    out = tvlqr_backward_vjp(*(ops[name] for name in OPS[:4]), *fwd[:4], status, **ups, C_final=ops["Cfin"], c_final=ops["cfin"])
    torch.cuda.synchronize()
    return {name: g for name, g in zip(g64.GRADS, out[:6]) if g is not None}, out[6]


def _expanded(ops, B, T):
    """``ops`` with every shared axis written out: [B, T, ...] ([B, ...] for the final cost)."""
    out = {}
    for name, a in ops.items():
        if a is None:
            out[name] = None
            continue
        full = 4 if name in ("F", "C") else 3 if name in ("f", "c", "Cfin") else 2
        if a.ndim < full:
            a = np.repeat(a[None], B, axis=0)
        if name in OPS[:4] and a.shape[1] == 1:
            a = np.repeat(a, T, axis=1)
        out[name] = a
    return out


def _refs(ops, ups):
    return g64.references(*(ops[name] for name in OPS), ups)


def _own(ops, ups, fwd):
    return g64.own_forward(*(ops[name] for name in OPS), ups, fwd)


# ---- the budget rule -----------------------------------------------------------------------------------------------------

BUDGET_CASES = ([(n, m, 7, "wave16") for n, m in ((1, 1), (3, 2), (3, 5), (16, 8), (16, 16))]
                + [(n, m, 7, "wave32") for n, m in ((17, 8), (16, 17), (5, 20), (20, 10))] + [(32, 32, 4, "wave32")]
                + [(n, m, T, "wave16") for n, m in ((16, 8), (12, 5)) for T in (1, 2, 3)])


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("n,m,T,kernel", BUDGET_CASES)
def test_every_gradient_is_within_the_budget(n, m, T, kernel, final):
    """(32, 32): the augmented matrix is 65 columns wide, a lane carries two; T <= 3 at the default final cost: the last
    step reads C_{T-1} with row stride d."""
    assert _name(n, m, T) == "tvb_vjp_f64_" + kernel
    ops, ups = _problem(n, m, T, final=final)
    got, fwd = _autograd(ops, ups)
    refs = _refs(ops, ups)
    _MEASURED[f"({n},{m},{T}) final={final}"] = g64.check(got, refs, own=_own(ops, ups, fwd), what=f"({n},{m},{T}) final={final}")


@pytest.mark.parametrize("seed", [0, 1])
def test_the_long_unscaled_horizon_is_within_the_budget(seed):
    ops, ups = _problem(16, 8, 50, seed=seed, unscaled=True)
    got, fwd = _autograd(ops, ups)
    refs = _refs(ops, ups)
    _MEASURED[f"unscaled (16,8,50) seed {seed}"] = g64.check(got, refs, own=_own(ops, ups, fwd), what=f"unscaled seed {seed}")


@pytest.mark.parametrize("only", g64.UPS)
@pytest.mark.parametrize("n,m", [(16, 8), (5, 3)])
def test_each_upstream_gradient_alone(n, m, only):
    """The other four upstream pointers are NULL (``set_materialize_grads(False)``)."""
    ops, ups = _problem(n, m, 5, final=n == 5, only=(only,))
    assert sum(g is not None for g in ups.values()) == 1
    got, fwd = _autograd(ops, ups)
    g64.check(got, _refs(ops, ups), own=_own(ops, ups, fwd), what=f"({n},{m}) {only} alone")


def test_all_upstream_null_gives_exact_zeros():
    ops, _ = _problem(16, 8, 4, final=True)
    fwd, status = _forward(ops)
    grads, st = _vjp(ops, fwd, status, {})
    assert len(grads) == 6 and not st.any()
    for name, g in grads.items():
        assert g.dtype == F64 and not g.any(), name


def test_the_value_loss_over_many_x0():
    """sum over 64 draws of x0 of x0' V_0 x0 / 2 + v_0' x0 + const_0, one recursion and one sweep for all of them."""
    n, m, T, B = 16, 8, 20, 4
    ops, _ = _problem(n, m, T, B)
    x0 = np.random.default_rng(3).normal(size=(B, 64, n))
    leaves = _leaves(ops)
    K, k, V, v, const = tvlqr_backward(*(leaves[name] for name in OPS), dtype=F64)
    x = torch.as_tensor(x0, device="cuda")
    loss = (0.5 * torch.einsum("bsi,bij,bsj->", x, V[:, 0], x) + torch.einsum("bsi,bi->", x, v[:, 0, :, 0]) + 64 * const[:, 0].sum())
    loss.backward()
    torch.cuda.synchronize()
    got = {GRAD_OF[name]: t.grad.cpu().numpy() for name, t in leaves.items() if t is not None}
    ups = dict(gK=None, gk=None, gV=np.zeros((B, T, n, n)), gv=np.zeros((B, T, n)), gconst=np.zeros((B, T)))
    ups["gV"][:, 0] = 0.5 * np.einsum("bsi,bsj->bij", x0, x0)
    ups["gv"][:, 0] = x0.sum(1)
    ups["gconst"][:, 0] = 64.0
    g64.check(got, _refs(ops, ups), own=_own(ops, ups, _host_fwd((K, k, V, v, const))), what="value loss over 64 x0")


def test_gradcheck():
    """torch's defaults.  C enters as a symmetric matrix (an asymmetric one is refused), so it is differentiated through
    (A + A') / 2."""
    ops, _ = _problem(3, 2, 3, B=2)
    F, f, A, c = (torch.as_tensor(ops[name], device="cuda", dtype=F64).requires_grad_() for name in OPS[:4])

    def fn(F, f, A, c):
        return tvlqr_backward(F, f, 0.5 * (A + A.transpose(-1, -2)), c, dtype=F64)

    assert torch.autograd.gradcheck(fn, (F, f, A, c))


# ---- sharing -------------------------------------------------------------------------------------------------------------

def _share(ops, mode):
    """``ops`` ([B, T, ...]) with the operands of ``mode`` shared: (operands, names summed over the batch, over time)."""
    o = dict(ops)
    if mode == "batch":
        o.update(F=ops["F"][0], f=ops["f"][0], C=ops["C"][0])
        return o, ("F", "f", "C"), ()
    if mode == "time":
        o.update(F=ops["F"][:, :1], f=ops["f"][:, :1], C=ops["C"][:, :1])
        return o, (), ("F", "f", "C")
    if mode == "both":
        o.update(F=ops["F"][0, :1], f=ops["f"][0, :1], C=ops["C"][0, :1])
        return o, ("F", "f", "C"), ("F", "f", "C")
    if mode == "F":
        o.update(F=ops["F"][0])
        return o, ("F",), ()
    if mode == "Cc":
        o.update(C=ops["C"][0], c=ops["c"][0])
        return o, ("C", "c"), ()
    if mode == "f":
        o.update(f=ops["f"][0])
        return o, ("f",), ()
    assert mode == "final"
    o.update(Cfin=ops["Cfin"][0], cfin=ops["cfin"][0])
    return o, ("Cfin", "cfin"), ()


@pytest.mark.parametrize("mode", ["batch", "time", "both", "F", "Cc", "f", "final"])
@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_shared_operands_get_summed_gradients(n, m, mode):
    """Summed gradients under the summed budget; a time-summed gradient is, bit for bit, the sequential fp64 sum of the
    per-step bits of a time-strided call on the same forward; repeated calls give the same bits."""
    T, B = 5, 4
    full, ups = _problem(n, m, T, B, final=mode in ("final", "time"))
    ops, over_b, over_t = _share(full, mode)
    ops = {k: (None if a is None else np.ascontiguousarray(a)) for k, a in ops.items()}
    ex = _expanded(ops, B, T)
    got, fwd = _autograd(ops, ups)
    refs, own = _refs(ex, ups), _own(ex, ups, fwd)
    for name in OPS:
        if ops[name] is None:
            continue
        key = GRAD_OF[name]
        assert got[key].shape == ops[name].shape
        if name in over_b or name in over_t:
            g64.check_summed(got[key], refs, key, own, batch=name in over_b, time=name in over_t, what=f"({n},{m}) {mode}")
        else:
            g64.check({key: got[key]}, refs, own=own, names=(key,), what=f"({n},{m}) {mode}")
    again, _ = _autograd(ops, ups)
    for key in got:
        assert np.array_equal(got[key], again[key]), key
    if over_t and not over_b:
        outs, status = _forward(ops)
        summed, _ = _vjp(ops, outs, status, ups)
        steps, _ = _vjp(ex, outs, status, ups)
        for name in over_t:
            key = GRAD_OF[name]
            assert np.array_equal(summed[key].cpu().numpy().reshape(got[key].shape), got[key]), key
            per_step = steps[key].cpu().numpy()
            acc = per_step[:, 0].copy()
            for t in range(1, T):
                acc = per_step[:, t] + acc
            assert np.array_equal(summed[key].cpu().numpy()[:, 0], acc), key


@pytest.mark.parametrize("n,m,T,B", [(16, 8, 3, 131), (20, 10, 3, 65), (3, 2, 2, 16449)])
def test_a_batch_summed_gradient_is_the_emulated_sum_of_the_per_instance_bits(n, m, T, B):
    """F, f, C and the final cost's matrix shared by the batch (c, c_final per instance): chunks of 64 instances, one past
    a chunk, and (16 449 = 257 x 64 + 1) more chunks than the tree is wide.  F also with a time axis of 1: its record is
    the time sum, then summed over the batch."""
    one, _ = _problem(n, m, T, 1, final=True)
    rng = np.random.default_rng(B)
    ups = {k: v.astype(np.float64) for k, v in gref.upstream(n, m, T, B, seed=B).items()}
    ops = dict(F=one["F"][0], f=one["f"][0], C=one["C"][0], c=rng.normal(size=(B, T, n + m)), Cfin=one["Cfin"][0],
               cfin=rng.normal(size=(B, n)))
    fwd, status = _forward(ops)
    summed, st = _vjp(ops, fwd, status, ups)
    assert not st.any()
    per, _ = _vjp(_expanded(ops, B, T), fwd, status, ups)
    for key in ("dF", "df", "dC", "dCfin"):
        want = sum64.steady_state_sum(per[key].cpu().numpy())
        assert np.array_equal(summed[key].cpu().numpy().reshape(want.shape), want), key
    for key in ("dc", "dcfin"):
        assert same(summed[key], per[key]), key
    again, _ = _vjp(ops, fwd, status, ups)
    assert all(same(summed[key], again[key]) for key in summed)
    held = dict(ops, F=ops["F"][:1] * 1.0)
    fwd_h, status_h = _forward(held)
    both, _ = _vjp(held, fwd_h, status_h, ups)
    per_h, _ = _vjp(_expanded(held, B, T), fwd_h, status_h, ups)
    steps = per_h["dF"].cpu().numpy()
    acc = steps[:, 0].copy()
    for t in range(1, T):
        acc = steps[:, t] + acc
    assert np.array_equal(both["dF"].cpu().numpy()[0], sum64.steady_state_sum(acc))


def test_a_batch_summed_gradient_with_a_padded_time_stride():
    """Through the C ABI: dF summed over the batch into rows of twice its size.  The tree stage 2 then runs once per step;
    the bits are the dense call's and the padding is not touched."""
    n, m, T, B = 5, 3, 4, 70
    d, size = n + m, n * (n + m)
    ops, ups = _problem(n, m, T, B)
    ops["F"] = ops["F"][0]
    fwd, status = _forward(ops)
    dense, _ = _vjp(ops, fwd, status, ups)
    lib = _hip.load()
    tv = TimeVaryingLQR(*(ops[name] for name in OPS), device="cuda", dtype=F64)
    up = [torch.as_tensor(ups[name], device="cuda").contiguous() for name in g64.UPS]
    out = torch.full((T, 2 * size), float("nan"), device="cuda", dtype=F64)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(B, n, m, T))
    ws = torch.empty(ws_bytes // 8, device="cuda", dtype=F64)
    rc = lib.tfmpc_tvlqr_backward_vjp_f64(B, n, m, T, *tv._model_args(), *(_hip.ptr(t) for t in fwd[:4]), _hip.ptr(status),
                                          *(_hip.ptr(u) for u in up), _hip.ptr(out), 0, 2 * size, None, 0, 0, None, 0, 0,
                                          None, 0, 0, None, 0, None, 0, _hip.ptr(st), _hip.ptr(ws), ws_bytes, _hip.stream())
    torch.cuda.synchronize()
    assert rc == 0 and not st.any()
    assert same(out[:, :size].reshape(T, n, d), dense["dF"]) and torch.isnan(out[:, size:]).all()


def test_an_instance_has_the_same_bits_alone_and_deep_in_a_batch():
    n, m, T, B, at = 16, 8, 3, 4096, 4000
    ops, ups = _problem(n, m, T, 64, seed=11, final=True)           # 64 distinct instances, tiled
    ops = {k: np.tile(a, (B // 64,) + (1,) * (a.ndim - 1)) for k, a in ops.items()}
    ups = {k: np.tile(g, (B // 64,) + (1,) * (g.ndim - 1)) for k, g in ups.items()}
    fwd, status = _forward(ops)
    big, _ = _vjp(ops, fwd, status, ups)
    one = {k: a[at:at + 1] for k, a in ops.items()}
    fwd1, status1 = _forward(one)
    for a, b in zip(fwd, fwd1):
        assert same(a[at:at + 1], b)
    alone, _ = _vjp(one, fwd1, status1, {k: g[at:at + 1] for k, g in ups.items()})
    for key in big:
        assert same(big[key][at:at + 1], alone[key]), key
    again, _ = _vjp(ops, fwd, status, ups)
    assert all(same(big[key], again[key]) for key in big)


# ---- status --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(16, 8), (5, 3), (20, 10)])
def test_a_flagged_instance_is_isolated(n, m):
    T, B, bad = 5, 4, 1
    ops, ups = _problem(n, m, T, B, final=True)
    ops["C"][bad, :, n:, n:] = -1e3 * np.eye(m)
    fwd, status = _forward(ops)
    assert status.tolist() == [0, ST_NOT_PD, 0, 0]
    grads, st = _vjp(ops, fwd, status, ups)
    assert st.tolist() == [0, ST_NOT_PD, 0, 0]
    keep = [b for b in range(B) if b != bad]
    rest = {k: a[keep] for k, a in ops.items()}
    fwd_r, status_r = _forward(rest)
    clean, st_r = _vjp(rest, fwd_r, status_r, {k: g[keep] for k, g in ups.items()})
    assert not st_r.any()
    for key, g in grads.items():
        assert torch.isnan(g[bad]).all(), key
        assert same(g[keep], clean[key]), key                      # the neighbours' bits: those of a run without it
    shared = dict(ops, F=ops["F"][0], f=ops["f"][0], Cfin=ops["Cfin"][0])      # every sum that contains it is NaN
    fwd_s, status_s = _forward(shared)
    sums, st_s = _vjp(shared, fwd_s, status_s, ups)
    assert st_s.tolist() == [0, ST_NOT_PD, 0, 0]
    for key in ("dF", "df", "dCfin"):
        assert torch.isnan(sums[key]).all(), key
    assert torch.isnan(sums["dC"][bad]).all() and not torch.isnan(sums["dC"][keep]).any()
    # flagged by the backward alone: a forward that says OK, one instance's V far from positive definite
    good, _ = _problem(n, m, T, B, final=True)
    fwd_g, status_g = _forward(good)
    assert not status_g.any()
    V = fwd_g[2].clone()
    V[bad] = -1e6 * torch.eye(n, device="cuda", dtype=F64)
    grads, st = _vjp(good, (fwd_g[0], fwd_g[1], V, fwd_g[3]), status_g, ups)
    assert st.tolist() == [0, ST_NOT_PD, 0, 0]
    ok, _ = _vjp(good, fwd_g, status_g, ups)
    for key, g in grads.items():
        assert torch.isnan(g[bad]).all() and same(g[keep], ok[key][keep]), key


# ---- the bits that must not move -----------------------------------------------------------------------------------------

def test_forward_bits_are_the_double_recursions():
    ops, _ = _problem(16, 8, 6, final=True)
    policy, value = TimeVaryingLQR(*(ops[name] for name in OPS), device="cuda", dtype=F64).backward()
    want = (policy.K, policy.k, value.V, value.v, value.const)
    leaves = _leaves(ops)
    for outs in (tvlqr_backward(*leaves.values(), dtype=F64), tvlqr_backward(*ops.values(), dtype=F64)):
        for a, b in zip(outs, want):
            assert same(a.detach(), torch.as_tensor(b, device="cuda"))
    one = tvlqr_backward(*(None if a is None else torch.as_tensor(a[0]) for a in ops.values()), dtype=F64)      # no batch axis
    assert tuple(one[0].shape) == (6, 8, 16) and same(one[0], torch.as_tensor(want[0], device="cuda")[0])


def test_the_fp32_path_is_unchanged():
    ops, ups = _problem(16, 8, 6, final=True)
    ops32 = {k: a.astype(np.float32) for k, a in ops.items()}
    runs = []
    for call in ("function", "function32", "method"):
        leaves = {k: torch.as_tensor(a, device="cuda").requires_grad_() for k, a in ops32.items()}
        if call == "method":
            policy, value = TimeVaryingLQR(*leaves.values()).backward(differentiable=True)
            outs = (policy.K, policy.k, value.V, value.v, value.const)
        else:
            outs = tvlqr_backward(*leaves.values(), **(dict(dtype=torch.float32) if call == "function32" else {}))
        assert all(o.dtype == torch.float32 for o in outs)
        _loss(outs, {k: g.astype(np.float32) for k, g in ups.items()}).backward()
        torch.cuda.synchronize()
        runs.append([o.detach() for o in outs] + [t.grad for t in leaves.values()])
    for other in runs[1:]:
        assert all(same(a, b) for a, b in zip(runs[0], other))


@pytest.mark.parametrize("seed", [0, 1])
def test_against_the_fp32_path(seed):
    """Unscaled (16, 8), T = 50, per instance: the fp32 path's error against the 80-bit closed form is at least 1e4 times
    the double path's (floored at 2^-48 of the gradient's scale) on dF and dC.  df and dc are printed, not asserted."""
    ops, ups = _problem(16, 8, 50, seed=seed, unscaled=True)
    got64, _ = _autograd(ops, ups)
    leaves32 = {k: (None if a is None else torch.as_tensor(a, device="cuda", dtype=torch.float32).requires_grad_())
                for k, a in ops.items()}
    outs = tvlqr_backward(*leaves32.values())
    _loss(outs, {k: g.astype(np.float32) for k, g in ups.items()}).backward()
    torch.cuda.synchronize()
    rld = _refs(ops, ups)[0]
    for name in ("F", "f", "C", "c"):
        key = GRAD_OF[name]
        err32 = g64._err(leaves32[name].grad.double().cpu().numpy(), rld[key], 1)
        err64 = np.maximum(g64._err(got64[key], rld[key], 1), g64.FLOOR * g64._scale(rld[key], 1))
        gain = err32 / err64
        print(f"fp32 error / fp64 error, unscaled seed {seed} {key}: min {gain.min():.3g} median {np.median(gain):.3g}")
        if key in ("dF", "dC"):
            assert gain.min() >= 1e4, (key, gain)


# ---- stale memory (tests/stale_memory.py) -----------------------------------------------------------------------------------

@pytest.mark.parametrize("shared", [(), ("F", "C"), OPS[:4]], ids=["per", "shared-F-C", "unbatched"])
@pytest.mark.parametrize("n,m", [(1, 1), (16, 8), (20, 10)])
def test_no_stale_memory_is_read_or_left(n, m, shared):
    T, B = 4, 3
    ops, ups = _problem(n, m, T, B)
    ops = {k: (a[0] if k in shared else a) for k, a in ops.items() if a is not None}
    Bk = 1 if len(shared) == 4 else B
    ups = {k: g[:Bk] for k, g in ups.items()}
    workspace_bytes = int(_hip.load().tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(Bk, n, m, T)) if 0 < len(shared) < 4 else 0

    def call():
        outs = tvlqr_backward(*ops.values(), dtype=F64)
        tv = TimeVaryingLQR(*ops.values(), device="cuda", dtype=F64)
        fwd = tv._backward_launch()
        grads = tvlqr_backward_vjp(*ops.values(), *fwd[:4], fwd[5], **ups)
        tensors = dict(zip(OUTS, outs))
        tensors.update({name: g for name, g in zip(g64.GRADS, grads[:4])})
        return tensors, list(tensors)

    runs = []
    for i, pattern in enumerate(PATTERNS):
        with StaleMemory(pattern, seed=17 * i) as mem:
            tensors, made = call()
            torch.cuda.synchronize()
        mem.check({k: tensors[k] for k in made}, workspace_bytes)
        runs.append({k: v.detach().clone() for k, v in tensors.items()})
    tensors, _ = call()
    torch.cuda.synchronize()
    runs.append({k: v.detach().clone() for k, v in tensors.items()})
    for label, other in zip(PATTERNS[1:] + ("unpatched",), runs[1:]):
        for k in runs[0]:
            assert same(runs[0][k], other[k]), (k, label)
    assert all(torch.isfinite(v).all() for v in runs[0].values())
