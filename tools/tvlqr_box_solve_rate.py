"""Rate of the control-limited TV-LQR forward (tfmpc_tvlqr_box_solve_f32) beside the control-limited iLQR
launch (box_lqr_solve's forward) on the same problem, in the same run.

    python tools/tvlqr_box_solve_rate.py [--batch 65536] [--out profiles/tvlqr_box_solve_rate.json]

B x (n = 16, m = 8, T = 50), the numbers of workloads.control_limited_stable, device events, 40 untimed calls of every
line, then 10 timed rounds that run the lines one after the other (alternating); the median per line.  Lines:
  (a) newton_stride0       the time-invariant model through stride-0 operands (time stride 0)
  (b) newton_materialised  the same numbers materialised per step and per instance ([B, T, ...])
  (c) ilqr                 iLQR(LQEnv).solve_device at atol = 1e-6, what box_lqr_solve runs forward
and the distribution of `iterations` (backward sweeps per instance) of (a), its status bits, the instances that end
flagged as failed beside what the iLQR launch says of them, and the iLQR launch's own flagged count.  No time bar is set."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests")]
from tfmpc import _hip  # noqa: E402


def timed_alternating(fns, warm=40, reps=10):
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _hip.require_gpu()
    import workloads
    B, n, m, T = args.batch, 16, 8, 50
    dev = "cuda"
    w = workloads.control_limited_stable(B, n, m, T, 0.5)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev).contiguous()      # noqa: E731
    F, f, C, c = (t(w[k]) for k in ("F", "f", "C", "c"))
    x0 = w["x0"].reshape(B, n).contiguous()
    low, high = torch.full((m,), -0.5, device=dev), torch.full((m,), 0.5, device=dev)
    out = dict(states=torch.empty(B, T + 1, n, device=dev), actions=torch.empty(B, T, m, device=dev),
               costs=torch.empty(B, T + 1, device=dev))
    iterations, status, reason = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    ws = torch.empty((lib.tfmpc_tvlqr_box_solve_workspace_bytes(B, n, m, T) + 3) // 4, device=dev)

    def launch(ops, time_strided):
        model = []
        for a in ops:
            model += [_hip.ptr(a), a[0].numel(), a[0, 0].numel() if time_strided else 0]
        rc = lib.tfmpc_tvlqr_box_solve_f32(B, n, m, T, *model, None, 0, None, 0, _hip.ptr(low), 0, 0, _hip.ptr(high), 0, 0,
                                           _hip.ptr(x0), None, 0, 0, 0.0, _hip.ptr(out["states"]), _hip.ptr(out["actions"]),
                                           _hip.ptr(out["costs"]), _hip.ptr(iterations), _hip.ptr(status), _hip.ptr(reason), None,
                                           _hip.ptr(ws), ws.numel() * 4, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_box_solve_f32")

    full = [a.unsqueeze(1).expand(B, T, *a.shape[1:]).contiguous() for a in (F, f, C, c)]
    solver = workloads.solver_of(w, atol=1e-6)
    hold = {}
    fns = dict(newton_stride0=lambda: launch((F, f, C, c), False),
               newton_materialised=lambda: launch(full, True),
               ilqr=lambda: hold.update(solver.solve_device(w["x0"], T, u_init=w["u0"], workspace=hold.get("workspace"))))
    ms = timed_alternating(fns, warm=args.warm)
    fns["newton_stride0"]()
    torch.cuda.synchronize()
    it = iterations.cpu().numpy()
    ilqr_it = hold["iterations"].cpu().numpy().reshape(-1)
    st, rs = status.cpu().numpy(), reason.cpu().numpy()
    bits = dict(NOT_PD=2, NAN=4, QP_MAXITER=8, MAX_ATTEMPTS=16)
    failed = np.nonzero(rs == 3)[0]
    ilqr_st = hold["status"].cpu().numpy().reshape(-1)
    result = dict(B=B, n=n, m=m, T=T, workload=w["version"], kernel=lib.tfmpc_tvlqr_box_solve_kernel_name(n, m, T).decode(),
                  ms=ms, ratio_newton_stride0_over_ilqr=ms["newton_stride0"] / ms["ilqr"],
                  iterations_histogram=np.bincount(it).tolist(), iterations_median=float(np.median(it)), iterations_max=int(it.max()),
                  flagged=int((st != 0).sum()), reasons=np.bincount(rs, minlength=4).tolist(),
                  status_bits={k: int((st & v != 0).sum()) for k, v in bits.items()},
                  failed_instances=[dict(instance=int(b), status=int(st[b]), iterations=int(it[b]), ilqr_status=int(ilqr_st[b]),
                                         ilqr_iterations=int(ilqr_it[b])) for b in failed[:32]],
                  ilqr_flagged=int((ilqr_st != 0).sum()),
                  ilqr_iterations_median=float(np.median(ilqr_it)), ilqr_iterations_max=int(ilqr_it.max()),
                  method=f"device events, {args.warm} untimed calls per line, median of 10 alternating rounds")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
