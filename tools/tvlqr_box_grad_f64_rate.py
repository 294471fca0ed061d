"""Rate of the double-precision control-limited TV-LQR VJP (tfmpc_tvlqr_box_vjp_f64) beside the plain double
VJP (tfmpc_tvlqr_vjp_f64) on the same operands and the double control-limited forward (tfmpc_tvlqr_box_solve_f64), in the
same run.

    python tools/tvlqr_box_grad_f64_rate.py [--batch 65536] [--out profiles/tvlqr_box_grad_f64_rate.json]

The method of tools/tvlqr_box_grad_rate.py and tools/tvlqr_grad_rate.py: B x (n = 16, m = 8, T = 50), the numbers of
workloads.control_limited_stable handed to the double kernels as doubles, the trajectory and the held set of the double
forward itself, mixed loss, every gradient requested, dlow / dhigh shared by the batch; device events, 40 untimed calls of
every line, then 10 timed rounds that run the lines one after the other (alternating); the median per line.  Lines: (a)
per-instance models, the time-invariant model written out per step as the VJP's per-step outputs want it, (b) one model
(instance 0's) shared by the batch.  The plain VJP is handed the v of tfmpc_tvlqr_solve_f64 on the same operands.  No time
bar is set.  --once: one call of each launch sequence, for a kernel trace."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from tfmpc import _hip  # noqa: E402
from tvlqr_box_solve_rate import timed_alternating  # noqa: E402

F64 = torch.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true", help="one call of each launch sequence (for a kernel trace)")
    args = ap.parse_args()
    lib = _hip.require_gpu()
    import workloads
    B, n, m, T = args.batch, 16, 8, 50
    d = n + m
    dev = "cuda"
    w = workloads.control_limited_stable(B, n, m, T, 0.5)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev).to(F64).contiguous()      # noqa: E731
    inv = [t(w[k]) for k in ("F", "f", "C", "c")]                     # [B, ...]: the time-invariant model
    x0 = w["x0"].reshape(B, n).to(F64).contiguous()
    low, high = torch.full((m,), -0.5, dtype=F64, device=dev), torch.full((m,), 0.5, dtype=F64, device=dev)
    states, actions = torch.empty(B, T + 1, n, dtype=F64, device=dev), torch.empty(B, T, m, dtype=F64, device=dev)
    costs = torch.empty(B, T + 1, dtype=F64, device=dev)
    iterations, fstatus, reason = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    fws = torch.empty(lib.tfmpc_tvlqr_box_solve_workspace_bytes_f64(B, n, m, T) // 8 + 1, dtype=F64, device=dev)

    def forward():
        model = []
        for a in inv:
            model += [_hip.ptr(a), a[0].numel(), 0]
        rc = lib.tfmpc_tvlqr_box_solve_f64(B, n, m, T, *model, None, 0, None, 0, _hip.ptr(low), 0, 0, _hip.ptr(high), 0, 0, _hip.ptr(x0),
                                           None, 0, 0, 0.0, _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs), _hip.ptr(iterations),
                                           _hip.ptr(fstatus), _hip.ptr(reason), None, _hip.ptr(fws), fws.numel() * 8, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_box_solve_f64")

    forward()
    torch.cuda.synchronize()
    good = fstatus == 0                                               # (a flagged instance has NaN rows: it keeps its x0, u = 0)
    states[~good], actions[~good] = 0.0, 0.0
    traj = (states.clone(), actions.clone())
    gen = torch.Generator(device=dev).manual_seed(0)
    g = tuple(torch.randn(*s, device=dev, generator=gen, dtype=F64) for s in ((B, T + 1, n), (B, T, m), (B, T + 1)))
    result = dict(B=B, n=n, m=m, T=T, workload=w["version"], dtype="float64", kernel=lib.tfmpc_tvlqr_box_vjp_kernel_name_f64(n, m, T).decode(),
                  held_fraction=float(((traj[1] == -0.5) | (traj[1] == 0.5)).double().mean()), forward_flagged=int((~good).sum()),
                  box_vjp_workspace_bytes=int(lib.tfmpc_tvlqr_box_vjp_workspace_bytes_f64(B, n, m, T)), lines={},
                  method=f"device events, {args.warm} untimed calls per line, median of 10 alternating rounds")
    for line, Bm in (("per_instance", B), ("shared", 1)):
        ops = [a[:Bm].unsqueeze(1).expand(Bm, T, *a.shape[1:]).contiguous() for a in inv]      # [Bm, T, ...]
        sb = lambda a: a[0].numel() if Bm > 1 else 0                  # noqa: E731
        model = []
        for a in ops:
            model += [_hip.ptr(a), sb(a), a[0, 0].numel()]
        model += [None, 0, None, 0]
        grads = [torch.empty_like(a) for a in ops]
        outs = []
        for a in grads:
            outs += [_hip.ptr(a), sb(a), a[0, 0].numel()]
        dx0 = torch.empty(B, n, dtype=F64, device=dev)
        outs += [None, 0, None, 0, _hip.ptr(dx0), n]
        dlow, dhigh = torch.empty(m, dtype=F64, device=dev), torch.empty(m, dtype=F64, device=dev)
        status, pstatus = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        ws = torch.empty(lib.tfmpc_tvlqr_box_vjp_workspace_bytes_f64(B, n, m, T) // 8 + 1, dtype=F64, device=dev)
        # the plain VJP's extra input: the v of the unconstrained solve on the same operands
        v = torch.empty(B, T, n, dtype=F64, device=dev)
        sx, su, sc = torch.empty_like(states), torch.empty_like(actions), torch.empty_like(costs)
        rc = lib.tfmpc_tvlqr_solve_f64(B, n, m, T, *model, _hip.ptr(x0), _hip.ptr(sx), _hip.ptr(su), _hip.ptr(sc), None, None, None,
                                       _hip.ptr(v), None, _hip.ptr(pstatus), _hip.ptr(ws), ws.numel() * 8, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_solve_f64")
        del sx, su, sc
        head = [B, n, m, T, *model]
        ups = [_hip.ptr(a) for a in g]
        tail = [_hip.ptr(ws), ws.numel() * 8, _hip.stream()]

        def plain():
            _hip.check(lib.tfmpc_tvlqr_vjp_f64(*head, _hip.ptr(traj[0]), _hip.ptr(traj[1]), _hip.ptr(v), *ups, *outs, _hip.ptr(pstatus),
                                               *tail), "tfmpc_tvlqr_vjp_f64")

        def box():
            _hip.check(lib.tfmpc_tvlqr_box_vjp_f64(*head, _hip.ptr(low), 0, 0, _hip.ptr(high), 0, 0, _hip.ptr(traj[0]), _hip.ptr(traj[1]),
                                                   *ups, *outs, _hip.ptr(dlow), 0, 0, _hip.ptr(dhigh), 0, 0, None, _hip.ptr(status), *tail),
                       "tfmpc_tvlqr_box_vjp_f64")

        if args.once:
            plain()
            box()
            if line == "per_instance":
                forward()
            torch.cuda.synchronize()
        else:
            fns = dict(box_vjp=box, plain_vjp=plain)
            if line == "per_instance":
                fns["box_solve"] = forward
            ms = timed_alternating(fns, warm=args.warm)
            torch.cuda.synchronize()
            result["lines"][line] = dict(ms=ms, box_over_plain=ms["box_vjp"] / ms["plain_vjp"], flagged=int((status != 0).sum()),
                                         finite=bool(all(torch.isfinite(a).all() for a in grads + [dlow, dhigh])))
            if "box_solve" in ms:
                result["lines"][line]["box_vjp_over_box_solve"] = ms["box_vjp"] / ms["box_solve"]
        del ops, grads, ws, v, model, outs, head
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out and not args.once:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
