"""Device-event times of the time-varying LQR (tfmpc_tvlqr_solve_f32) at B = 65 536, n = 16, m = 8, T = 50:

  (a) per-instance time-varying models (every instance streams its own 4 000 B per step: HBM-bound);
  (b) one time-varying model shared by the batch (L2-resident: compute-bound);
  (lqr) the time-invariant headline LQR (tfmpc_lqr_solve_f32) on the same shape, for scale;
  (ilqr_bw) what a user could run before: tfmpc_ilqr_backward_f32 (mu = 0, unbounded) on the same per-step models
        materialised as l_xx / l_uu / l_xu / l_x / l_u / f_x / f_u -- a backward pass only.

--dtype float64 times (a) and (b) on the double-precision path (tfmpc_tvlqr_solve_f64, DESIGN.md 3.14: 8 000 B per step),
keeps (lqr) and (ilqr_bw) -- fp32 only -- for scale, and adds the same run's fp32 (a) as a_per_instance_f32.

Prints one JSON object (median / min of --reps timed launches after --warmup) with the roofline fraction of (a) on
algorithmic bytes (the model read once per pass, two passes, plus trajectory and final cost).
Usage: python tools/tvlqr_rate.py [--dtype float32|float64] [--reps 20] [--warmup 3] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tvlqr_ref  # noqa: E402
from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402
from tfmpc.solvers.lqr import LQR  # noqa: E402

B, N, M, T = 65536, 16, 8, 50
POOL = 64                      # distinct instances; instance b stores a copy of pool[b % POOL]
SPEC_BW, MEASURED_BW = 8.0e12, 6.3e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    args = ap.parse_args()
    f64 = args.dtype == "float64"
    dt, size = (torch.float64, 8) if f64 else (torch.float32, 4)
    _hip.require_gpu()
    lib = _hip.load()
    d = N + M
    F, f, C, c = tvlqr_ref.make_models(N, M, T, POOL, seed=0)
    x0 = tvlqr_ref.make_x0(N, POOL)
    rep = lambda a: torch.as_tensor(a, device="cuda").repeat(B // POOL, *([1] * (a.ndim - 1)))   # noqa: E731
    Fd, fd, Cd, cd, x0d = rep(F), rep(f), rep(C), rep(c), rep(x0)[..., None]
    name = lib.tfmpc_tvlqr_kernel_name_f64 if f64 else lib.tfmpc_tvlqr_kernel_name
    res = dict(B=B, n=N, m=M, T=T, dtype=args.dtype, kernel=name(N, M, T).decode())

    def per_instance(dtype):
        tv = TimeVaryingLQR(Fd.to(dtype), fd.to(dtype), Cd.to(dtype), cd.to(dtype), device="cuda", symmetric=True, dtype=dtype)
        x0 = x0d.to(dtype)
        ws = tv.solve_device(x0)["workspace"]
        out = tv.solve_device(x0, workspace=ws)
        torch.cuda.synchronize()
        assert int(out["status"].abs().sum()) == 0
        return timed(lambda: tv.solve_device(x0, workspace=ws), args.reps, args.warmup), ws

    res["a_per_instance"], ws = per_instance(dt)
    shared = TimeVaryingLQR(*(torch.as_tensor(a[0], device="cuda") for a in (F, f, C, c)), device="cuda", symmetric=True, dtype=dt)
    x0t = x0d.to(dt)
    res["b_shared"] = timed(lambda: shared.solve_device(x0t, workspace=ws), args.reps, args.warmup)
    del ws
    if f64:
        res["a_per_instance_f32"] = per_instance(torch.float32)[0]

    lqr = LQR(Fd[:, 0].contiguous(), fd[:, 0, :, None].contiguous(), Cd[:, 0].contiguous(), cd[:, 0, :, None].contiguous(),
              device="cuda", symmetric=True)
    lws = torch.empty(int(lib.tfmpc_lqr_workspace_bytes(B, N, M, T)) // 4, device="cuda")
    res["lqr_headline"] = timed(lambda: lqr.solve_device(x0d, T, workspace=lws), args.reps, args.warmup)

    # the iLQR backward pass on the same models, materialised in its layouts
    f_x, f_u = Fd[..., :N].contiguous(), Fd[..., N:].contiguous()
    l_xx, l_uu, l_xu = Cd[..., :N, :N].contiguous(), Cd[..., N:, N:].contiguous(), Cd[..., :N, N:].contiguous()
    l_x, l_u = cd[..., :N].contiguous(), cd[..., N:].contiguous()
    l = torch.zeros((B, T), device="cuda")
    fl, fl_x, fl_xx = torch.zeros(B, device="cuda"), l_x[:, T - 1].contiguous(), l_xx[:, T - 1].contiguous()
    actions = torch.zeros((B, T, M), device="cuda")
    low, high = torch.full((M,), -1e30, device="cuda"), torch.full((M,), 1e30, device="cuda")
    mu = torch.zeros(1, device="cuda")
    K, k = torch.empty((B, T, M, N), device="cuda"), torch.empty((B, T, M), device="cuda")
    J, dV1, dV2 = (torch.empty(B, device="cuda") for _ in range(3))
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    P = _hip.ptr

    def ilqr_bw():
        rc = lib.tfmpc_ilqr_backward_f32(B, N, M, T, P(actions), P(f_x), P(f_u), P(l), P(l_x), P(l_u), P(l_xx), P(l_uu), P(l_xu),
                                         P(fl), P(fl_x), P(fl_xx), P(low), P(high), 0, P(mu), 0,
                                         P(K), P(k), P(J), P(dV1), P(dV2), P(status), _hip.stream())
        _hip.check(rc, "tfmpc_ilqr_backward_f32")
    res["ilqr_backward_baseline"] = timed(ilqr_bw, args.reps, args.warmup)

    model_bytes = T * size * (N * d + N + d * d + d)                    # 4 000 B per step in fp32, 8 000 B in double
    total = B * (2 * model_bytes + size * ((T + 1) * N + T * M + (T + 1) + N * N + N))
    ta = res["a_per_instance"]["median_ms"] * 1e-3
    res["roofline_a"] = dict(algorithmic_bytes=total, spec_ms=total / SPEC_BW * 1e3, achievable_ms=total / MEASURED_BW * 1e3,
                             fraction_of_spec=total / ta / SPEC_BW, achieved_TBps=total / ta / 1e12,
                             workspace_roundtrip_bytes_per_instance=2 * T * M * (N + 1) * size)
    res["b_over_lqr"] = res["b_shared"]["median_ms"] / res["lqr_headline"]["median_ms"]
    res["ilqr_over_a"] = res["ilqr_backward_baseline"]["median_ms"] / res["a_per_instance"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
