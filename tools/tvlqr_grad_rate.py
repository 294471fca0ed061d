"""Device-event times of the time-varying LQR's gradient (tfmpc_tvlqr_vjp_f32) at B = 65 536, n = 16, m = 8, T = 50:

  (a) per-instance time-varying models: forward solve, backward (fold + adjoint solve + VJP sweep);
  (b) one time-varying model shared by the batch: the same, gradients summed over the batch;
  (torch) autograd (forward + backward) through a batched fp32 torch restatement of the same recursion
          (tests/tvlqr_grad_ref.py) on the same GPU, for scale.

The backward is timed as one tfmpc_tvlqr_vjp_f32 call with a mixed loss (states, actions and costs) and every gradient
requested.  Prints one JSON object (median / min of --reps timed launches after --warmup) with the VJP sweep's
algorithmic bytes for (a): the model read once (4 000 B per step), each gradient written once, trajectory, adjoint
trajectory and c~ read once.  Per-kernel times come from a kernel trace (profiles/tvlqr_grad_*).

--dtype float64 times (a) and (b) on the double-precision path (tfmpc_tvlqr_solve_f64 with v requested,
tfmpc_tvlqr_vjp_f64): backward over the fp64 forward of the same run, the per-kernel times of one
backward (torch.profiler's device activity), and the costate-and-gradient kernel's time against its algorithmic bytes
-- V, v, v~, z, dz read once and every gradient written once -- at the 6.3 TB/s DESIGN.md 3.14 cites as achievable.
Usage: python tools/tvlqr_grad_rate.py [--dtype float32|float64] [--reps 20] [--warmup 3] [--torch-reps 3] [--out file.json]"""
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

import tvlqr_grad_ref  # noqa: E402
import tvlqr_ref  # noqa: E402
from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402
from tvlqr_rate import B, M, MEASURED_BW, N, POOL, SPEC_BW, T, timed  # noqa: E402


def vjp_call(lib, tv, out, ups, grads, ws, status):
    """One tfmpc_tvlqr_vjp_f32 launch sequence; grads: dict of contiguous buffers shaped like tv's operands."""
    args = []
    for name in ("F", "f", "C", "c"):
        g = grads[name]
        sb = g[0].numel() if g.dim() == 4 else 0
        st = g.shape[-2] * g.shape[-1] if g.shape[-3] > 1 else 0
        args += [_hip.ptr(g), sb, st]
    args += [None, 0, None, 0, _hip.ptr(grads["x0"]), N]
    rc = lib.tfmpc_tvlqr_vjp_f32(B, N, M, T, *tv._model_args(), _hip.ptr(out["states"]), _hip.ptr(out["actions"]),
                                 *(_hip.ptr(u) for u in ups), *args, _hip.ptr(status), _hip.ptr(ws), ws.numel() * 4,
                                 _hip.stream())
    _hip.check(rc, "tfmpc_tvlqr_vjp_f32")


def vjp_call_f64(lib, tv, out, ups, grads, ws, status):
    """vjp_call for tfmpc_tvlqr_vjp_f64: the forward's v goes in as well."""
    args = []
    for name in ("F", "f", "C", "c"):
        g = grads[name]
        sb = g[0].numel() if g.dim() == 4 else 0
        st = g.shape[-2] * g.shape[-1] if g.shape[-3] > 1 else 0
        args += [_hip.ptr(g), sb, st]
    args += [None, 0, None, 0, _hip.ptr(grads["x0"]), N]
    rc = lib.tfmpc_tvlqr_vjp_f64(B, N, M, T, *tv._model_args(), _hip.ptr(out["states"]), _hip.ptr(out["actions"]),
                                 _hip.ptr(out["v"]), *(_hip.ptr(u) for u in ups), *args, _hip.ptr(status), _hip.ptr(ws),
                                 ws.numel() * 8, _hip.stream())
    _hip.check(rc, "tfmpc_tvlqr_vjp_f64")


def kernel_times(fn, calls=3):
    """Mean device time in ms per kernel name over ``calls`` runs of ``fn``; None when the profiler reports no device activity."""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
            if total:
                out[e.key] = total / calls / 1e3
        return out or None
    except Exception as exc:        # noqa: BLE001  (a measurement aid: the event times above do not depend on it)
        return dict(error=repr(exc))


def main_f64(args):
    _hip.require_gpu()
    lib = _hip.load()
    d, f64 = N + M, torch.float64
    F, f, C, c = tvlqr_ref.make_models(N, M, T, POOL, seed=0)
    x0 = tvlqr_ref.make_x0(N, POOL)
    rep = lambda a: torch.as_tensor(a, device="cuda", dtype=f64).repeat(B // POOL, *([1] * (a.ndim - 1)))   # noqa: E731
    x0d = rep(x0)[..., None]
    rng = np.random.default_rng(0)
    ups = [torch.as_tensor(rng.normal(size=s), device="cuda") for s in ((B, T + 1, N), (B, T, M), (B, T + 1))]
    res = dict(B=B, n=N, m=M, T=T, dtype="float64", fp32_backward_over_forward=3.09)
    ws = torch.empty(int(lib.tfmpc_tvlqr_workspace_bytes_f64(B, N, M, T)) // 8, device="cuda", dtype=f64)
    vbytes = int(lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(B, N, M, T))
    vws = torch.empty(vbytes // 8, device="cuda", dtype=f64)
    res["vjp_workspace_bytes"] = vbytes
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    for key in ("a_per_instance", "b_shared"):
        if key == "a_per_instance":
            tv = TimeVaryingLQR(rep(F), rep(f), rep(C), rep(c), device="cuda", symmetric=True, dtype=f64)
        else:
            tv = TimeVaryingLQR(*(torch.as_tensor(a[0], device="cuda", dtype=f64) for a in (F, f, C, c)), device="cuda",
                                symmetric=True, dtype=f64)
        out = tv.solve_device(x0d, workspace=ws, want_v=True)
        grads = dict(F=torch.empty_like(tv.F), f=torch.empty_like(tv.f), C=torch.empty_like(tv.C), c=torch.empty_like(tv.c),
                     x0=torch.empty((B, N, 1), device="cuda", dtype=f64))
        vjp_call_f64(lib, tv, out, ups, grads, vws, status)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        fw = timed(lambda: tv.solve_device(x0d, workspace=ws, want_v=True), args.reps, args.warmup)
        bw = timed(lambda: vjp_call_f64(lib, tv, out, ups, grads, vws, status), args.reps, args.warmup)
        res[key] = dict(forward=fw, backward=bw, backward_over_forward=bw["median_ms"] / fw["median_ms"],
                        backward_kernels_ms=kernel_times(lambda: vjp_call_f64(lib, tv, out, ups, grads, vws, status)))
        del tv, out, grads
    # (a): algorithmic bytes of the costate-and-gradient kernel per (b, t): V_{t+1}, v_{t+1}, v~_{t+1}, x_{t+1}, dx_{t+1},
    # z_t, dz_t read once; dF_t, df_t, dC_t, dc_t written once; dx0 per instance (v~_0 read, dx0 written)
    read_step = 8 * (N * N + 2 * N + 2 * N + 2 * d)
    grad_step = 8 * (N * d + N + d * d + d)
    nbytes = B * (T * (read_step + grad_step) + 8 * 2 * N)
    res["costate_algorithmic_bytes_a"] = nbytes
    res["costate_achievable_ms_a"] = nbytes / MEASURED_BW * 1e3
    res["costate_spec_ms_a"] = nbytes / SPEC_BW * 1e3
    kt = res["a_per_instance"]["backward_kernels_ms"] or {}
    hit = [v for k, v in kt.items() if "vjp_costate_kernel" in k]
    if hit:
        res["costate_kernel_ms_a"] = sum(hit)
        res["costate_fraction_of_achievable_a"] = res["costate_achievable_ms_a"] / sum(hit)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    args = ap.parse_args()
    if args.dtype == "float64":
        return main_f64(args)
    _hip.require_gpu()
    lib = _hip.load()
    d = N + M
    F, f, C, c = tvlqr_ref.make_models(N, M, T, POOL, seed=0)
    x0 = tvlqr_ref.make_x0(N, POOL)
    rep = lambda a: torch.as_tensor(a, device="cuda").repeat(B // POOL, *([1] * (a.ndim - 1)))   # noqa: E731
    Fd, fd, Cd, cd, x0d = rep(F), rep(f), rep(C), rep(c), rep(x0)[..., None]
    rng = np.random.default_rng(0)
    ups = [torch.as_tensor(rng.normal(size=s).astype(np.float32), device="cuda")
           for s in ((B, T + 1, N), (B, T, M), (B, T + 1))]
    res = dict(B=B, n=N, m=M, T=T)
    ws = torch.empty(int(lib.tfmpc_tvlqr_workspace_bytes(B, N, M, T)) // 4, device="cuda")
    vws = torch.empty(int(lib.tfmpc_tvlqr_vjp_workspace_bytes(B, N, M, T)) // 4, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")

    for key, tv in (("a_per_instance", TimeVaryingLQR(Fd, fd, Cd, cd, device="cuda", symmetric=True)),
                    ("b_shared", TimeVaryingLQR(*(torch.as_tensor(a[0], device="cuda") for a in (F, f, C, c)),
                                                device="cuda", symmetric=True))):
        out = tv.solve_device(x0d, workspace=ws)
        grads = dict(F=torch.empty_like(tv.F), f=torch.empty_like(tv.f), C=torch.empty_like(tv.C), c=torch.empty_like(tv.c),
                     x0=torch.empty((B, N, 1), device="cuda"))
        vjp_call(lib, tv, out, ups, grads, vws, status)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        fw = timed(lambda: tv.solve_device(x0d, workspace=ws), args.reps, args.warmup)
        bw = timed(lambda: vjp_call(lib, tv, out, ups, grads, vws, status), args.reps, args.warmup)
        res[key] = dict(forward=fw, backward=bw, backward_over_forward=bw["median_ms"] / fw["median_ms"])

    # (a): algorithmic bytes of the VJP sweep -- model read once, gradients written once, z, dz, c~ read once
    model_step = 4 * (N * d + d * d + d)                   # F, C, c per step (f is not read by the sweep)
    grad_step = 4 * (N * d + N + d * d + d)
    traj_step = 4 * (2 * d + d)                            # z, dz, c~
    sweep_bytes = B * (T * (model_step + grad_step + traj_step) + 4 * 2 * N)
    res["sweep_algorithmic_bytes_a"] = sweep_bytes
    res["sweep_spec_ms_a"] = sweep_bytes / SPEC_BW * 1e3

    # torch autograd baseline: the same recursion, batched fp32 ops on the same GPU
    ops = [torch.as_tensor(a, device="cuda") for a in (F, f, C, c, x0)]
    ops = [o.repeat(B // POOL, *([1] * (o.dim() - 1))).requires_grad_() for o in ops]
    wx, wu, wc = ups

    def torch_fb():
        xs, us, cs = tvlqr_grad_ref.solve(*ops)
        loss = (xs * wx).sum() + (us * wu).sum() + (cs * wc).sum()
        torch.autograd.grad(loss, ops)
    res["torch_autograd_fp32"] = timed(torch_fb, args.torch_reps, 1)
    fb_a = res["a_per_instance"]["forward"]["median_ms"] + res["a_per_instance"]["backward"]["median_ms"]
    res["torch_over_a_forward_backward"] = res["torch_autograd_fp32"]["median_ms"] / fb_a
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
