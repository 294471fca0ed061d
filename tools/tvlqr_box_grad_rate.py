"""Rate of the control-limited TV-LQR VJP (tfmpc_tvlqr_box_vjp_f32) beside the plain VJP
(tfmpc_tvlqr_vjp_f32) on the same operands in the same run, and the control-limited forward for scale.

    python tools/tvlqr_box_grad_rate.py [--batch 65536] [--out profiles/tvlqr_box_grad_rate.json]

B x (n = 16, m = 8, T = 50), mixed loss, every gradient requested, device events, 40 untimed calls then the median of 10.
Lines: (a) per-instance models, (b) one model shared by the batch.  The operands are random (the launches' cost does not
depend on the values); half of the controls carry a bound's bits, which is what the held set is read from."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests")]
from tfmpc import _hip  # noqa: E402


def timed(fn, warm=40, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true", help="one call of each launch sequence (for a kernel trace)")
    args = ap.parse_args()
    lib = _hip.require_gpu()
    B, n, m, T = args.batch, 16, 8, 50
    d = n + m
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)      # noqa: E731
    result = dict(B=B, n=n, m=m, T=T, lines={})
    for line, Bm in (("per_instance", B), ("shared", 1)):
        F = rn(Bm, T, n, d) * (0.7 / np.sqrt(n))
        f = rn(Bm, T, n)
        A = rn(Bm, T, d, d)
        C = A @ A.transpose(-1, -2) / d + torch.eye(d, device=dev)
        del A
        c = rn(Bm, T, d)
        states, actions = rn(B, T + 1, n), rn(B, T, m).clamp(-0.67, 0.67)      # |N(0,1)| > 0.67 for half of the draws
        low, high = torch.full((m,), -0.67, device=dev), torch.full((m,), 0.67, device=dev)
        g = (rn(B, T + 1, n), rn(B, T, m), rn(B, T + 1))
        sb = lambda t: t[0].numel() if Bm > 1 else 0      # noqa: E731
        model = []
        for t in (F, f, C, c):
            model += [_hip.ptr(t), sb(t), t[0, 0].numel()]
        model += [None, 0, None, 0]
        grads = [torch.empty_like(t) for t in (F, f, C, c)]
        outs = []
        for t in grads:
            outs += [_hip.ptr(t), sb(t), t[0, 0].numel()]
        dx0 = torch.empty(B, n, device=dev)
        outs += [None, 0, None, 0, _hip.ptr(dx0), n]
        dlow, dhigh = torch.empty(m, device=dev), torch.empty(m, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        ws = torch.empty((lib.tfmpc_tvlqr_box_vjp_workspace_bytes(B, n, m, T) + 3) // 4, device=dev)
        head = [B, n, m, T, *model]
        mid = [_hip.ptr(states), _hip.ptr(actions), *(_hip.ptr(t) for t in g), *outs]
        tail = [_hip.ptr(status), _hip.ptr(ws), ws.numel() * 4, _hip.stream()]

        def plain():
            _hip.check(lib.tfmpc_tvlqr_vjp_f32(*head, *mid, *tail), "tfmpc_tvlqr_vjp_f32")

        def box():
            _hip.check(lib.tfmpc_tvlqr_box_vjp_f32(*head, _hip.ptr(low), 0, 0, _hip.ptr(high), 0, 0, *mid, _hip.ptr(dlow), 0, 0,
                                                   _hip.ptr(dhigh), 0, 0, None, *tail), "tfmpc_tvlqr_box_vjp_f32")

        if args.once:
            plain()
            box()
            torch.cuda.synchronize()
            continue
        t_plain, t_box = timed(plain), timed(box)
        held = float(((actions == -0.67) | (actions == 0.67)).float().mean())
        result["lines"][line] = dict(plain_ms=t_plain, box_ms=t_box, ratio=t_box / t_plain, held_fraction=held,
                                     target="box <= 1.15 x plain", met=bool(t_box <= 1.15 * t_plain),
                                     flagged=int((status != 0).sum()))
        del F, f, C, c, grads
        torch.cuda.empty_cache()
    if not args.once:
        import workloads
        from tfmpc.envs.lq import LQEnv
        from tfmpc.solvers.ilqr import iLQR
        w = workloads.control_limited_stable(B, n, m, T, 0.5)
        solver = iLQR(LQEnv(w["F"], w["f"], w["C"], w["c"], w["low"], w["high"]), atol=1e-6)
        hold = {}
        result["forward_ms"] = timed(lambda: hold.update(solver.solve_device(w["x0"], T, u_init=w["u0"], workspace=hold.get("workspace"))),
                                     warm=3, reps=5)
        result["forward"] = "iLQR(LQEnv) control-limited launch, workloads.control_limited_stable, atol = 1e-6"
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
