"""Device-event times of the Riccati recursion's gradient (tfmpc_tvlqr_backward_vjp_f32) at B = 65 536,
n = 16, m = 8, T = 50:

  (a) per-instance time-varying models: every gradient per instance and per step;
  (b) one time-varying model shared by the batch: the same, gradients summed over the batch (per-instance records in
      the workspace, then the two-stage reduction);
  (forward) tfmpc_tvlqr_backward_f32 with all value outputs on the same models, the yardstick.

All five upstream gradients are given and every gradient is requested.  Prints one JSON object (median / min of --reps
timed launches after --warmup untimed ones) with (a)'s algorithmic bytes: the model read once, K, k, V, v and the
upstream gradients read once, every gradient written once.

--dtype float64 times the double gradients (tfmpc_tvlqr_backward_vjp_f64) on lines (a) and (b): the double
VJP, the fp32 VJP and the double recursion (tfmpc_tvlqr_backward_f64) take turns in one process, 3 warm-up rounds and the
median of 20, the whole measurement twice (the gap between the two medians is the spread); one JSON line, written to
profiles/tvlqr_backward_grad_f64_rate.json unless --out names another file.
Usage: python tools/tvlqr_backward_grad_rate.py [--dtype float64] [--reps N] [--warmup N] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tvlqr_ref  # noqa: E402
from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402
from tvlqr_rate import B, M, N, POOL, SPEC_BW, T, timed  # noqa: E402


def vjp_call(lib, tv, fwd, ups, grads, ws, status):
    """One tfmpc_tvlqr_backward_vjp_f32 (_f64 for a double ``tv``) launch sequence; grads: contiguous buffers shaped like
    tv's operands."""
    sfx = "f64" if tv.dtype == torch.float64 else "f32"
    args = []
    for g in grads:
        sb = g[0].numel() if g.dim() == 4 else 0
        st = g.shape[-2] * g.shape[-1] if g.shape[-3] > 1 else 0
        args += [_hip.ptr(g), sb, st]
    entry = getattr(lib, "tfmpc_tvlqr_backward_vjp_" + sfx)
    rc = entry(B, N, M, T, *tv._model_args(), *(_hip.ptr(t) for t in fwd), *(_hip.ptr(u) for u in ups),
               *args, None, 0, None, 0, _hip.ptr(status), _hip.ptr(ws),
               0 if ws is None else ws.numel() * ws.element_size(), _hip.stream())
    _hip.check(rc, "tfmpc_tvlqr_backward_vjp_" + sfx)


def taking_turns(fns, reps, warmup):
    """name -> median ms of `reps` timed calls, the functions called one after the other in every round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: float(np.median(v)) for name, v in ts.items()}


def line_f64(lib, name, ops, ups, shared, reps, warmup):
    """One line of the double table: ``ops`` are fp32 cuda operands (F, f, C, c); the double problem is their upcast."""
    calls, keep = {}, []
    for dtype in (torch.float64, torch.float32):
        tv = TimeVaryingLQR(*(t.to(dtype) for t in ops), device="cuda", symmetric=True, dtype=dtype)
        K, k, V, v, _, fst = tv._backward_launch()
        fwd = (K, k, V, v, fst)
        grads = [torch.empty_like(t) for t in (tv.F, tv.f, tv.C, tv.c)]
        status = torch.empty(B, dtype=torch.int32, device="cuda")
        ws = None
        if shared:
            query = lib.tfmpc_tvlqr_backward_vjp_workspace_bytes_f64 if dtype == torch.float64 else lib.tfmpc_tvlqr_backward_vjp_workspace_bytes
            ws = torch.empty(int(query(B, N, M, T)) // dtype.itemsize, device="cuda", dtype=dtype)
        up = [u.to(dtype) for u in ups]
        call = (lambda tv=tv, fwd=fwd, up=up, grads=grads, ws=ws, status=status: vjp_call(lib, tv, fwd, up, grads, ws, status))
        call()
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0 and all(bool(torch.isfinite(g).all()) for g in grads)
        calls["vjp_f64" if dtype == torch.float64 else "vjp_f32"] = call
        if dtype == torch.float64:
            calls["forward_f64"] = tv._backward_launch
        keep.append((tv, fwd, grads, ws, up))
    fns = {key: calls[key] for key in ("vjp_f64", "vjp_f32", "forward_f64")}
    first, second = taking_turns(fns, reps, warmup), taking_turns(fns, reps, warmup)
    out = {}
    for key in fns:
        out[f"{name}_{key}_ms"] = first[key]
        out[f"{name}_{key}_repeat_ms"] = second[key]
        out[f"{name}_{key}_spread"] = abs(first[key] - second[key]) / min(first[key], second[key])
    out[f"{name}_vjp_f64_over_forward_f64"] = first["vjp_f64"] / first["forward_f64"]
    out[f"{name}_vjp_f64_over_vjp_f32"] = first["vjp_f64"] / first["vjp_f32"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    args = ap.parse_args()
    double = args.dtype == "float64"
    args.reps = args.reps if args.reps is not None else (20 if double else 10)
    args.warmup = args.warmup if args.warmup is not None else (3 if double else 40)
    _hip.require_gpu()
    lib = _hip.load()
    d = N + M
    F, f, C, c = tvlqr_ref.make_models(N, M, T, POOL, seed=0)
    rep = lambda a: torch.as_tensor(a, device="cuda").repeat(B // POOL, *([1] * (a.ndim - 1)))   # noqa: E731
    rng = np.random.default_rng(0)
    ups = [torch.as_tensor(rng.normal(size=s).astype(np.float32), device="cuda")
           for s in ((B, T, M, N), (B, T, M), (B, T, N, N), (B, T, N), (B, T))]
    res = dict(B=B, n=N, m=M, T=T, reps=args.reps, warmup=args.warmup,
               kernel=lib.tfmpc_tvlqr_backward_vjp_kernel_name(N, M, T).decode())
    status = torch.empty(B, dtype=torch.int32, device="cuda")

    if double:
        res.update(kernel=lib.tfmpc_tvlqr_backward_vjp_kernel_name_f64(N, M, T).decode(),
                   kernel_f32=lib.tfmpc_tvlqr_backward_vjp_kernel_name(N, M, T).decode(),
                   order="vjp_f64, vjp_f32, forward_f64 take turns; two runs of reps rounds")
        res.update(line_f64(lib, "a_per_instance", (rep(F), rep(f), rep(C), rep(c)), ups, False, args.reps, args.warmup))
        torch.cuda.empty_cache()
        cuda = lambda a: torch.as_tensor(a, device="cuda")      # noqa: E731
        res.update(line_f64(lib, "b_shared", (cuda(F[0]), cuda(f[0]), cuda(C[0]), rep(c)), ups, True, args.reps, args.warmup))
        line = json.dumps(res)
        print(line)
        with open(args.out or os.path.join(ROOT, "profiles", "tvlqr_backward_grad_f64_rate.json"), "w") as fh:
            fh.write(line + "\n")
        return

    for key, tv in (("a_per_instance", TimeVaryingLQR(rep(F), rep(f), rep(C), rep(c), device="cuda", symmetric=True)),
                    ("b_shared", TimeVaryingLQR(torch.as_tensor(F[0], device="cuda"), torch.as_tensor(f[0], device="cuda"),
                                                torch.as_tensor(C[0], device="cuda"), rep(c), device="cuda", symmetric=True))):
        # (b): F, f, C shared by the batch; c stays per instance -- it carries the batch axis -- and so does its gradient
        K, k, V, v, const, fst = tv._backward_launch()
        fwd = (K, k, V, v, fst)
        grads = [torch.empty_like(t) for t in (tv.F, tv.f, tv.C, tv.c)]
        shared = key == "b_shared"
        ws = None
        if shared:
            ws = torch.empty(int(lib.tfmpc_tvlqr_backward_vjp_workspace_bytes(B, N, M, T)) // 4, device="cuda")
        vjp_call(lib, tv, fwd, ups, grads, ws, status)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        assert all(bool(torch.isfinite(g).all()) for g in grads)
        fw = timed(tv._backward_launch, args.reps, args.warmup)
        bw = timed(lambda: vjp_call(lib, tv, fwd, ups, grads, ws, status), args.reps, args.warmup)
        res[key] = dict(forward=fw, vjp=bw, vjp_over_forward=bw["median_ms"] / fw["median_ms"])
        if shared:
            res[key]["workspace_bytes"] = ws.numel() * 4
        del grads, ws, fwd, K, k, V, v, const

    # (a): algorithmic bytes -- model read once (c is not read: the default final cost's c_{T-1} aside), K, k, V, v and the
    # upstream gradients read once, every gradient written once
    model_step = 4 * (N * d + N + d * d)
    fwd_step = 4 * (M * N + M + N * N + N)
    up_step = fwd_step + 4
    grad_step = 4 * (N * d + N + d * d + d)
    total = B * T * (model_step + fwd_step + up_step + grad_step)
    res["algorithmic_bytes_a"] = total
    res["spec_ms_a"] = total / SPEC_BW * 1e3
    res["a_over_spec"] = res["a_per_instance"]["vjp"]["median_ms"] / res["spec_ms_a"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
