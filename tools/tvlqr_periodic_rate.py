"""Rate of the periodic infinite-horizon LQR in double (tfmpc_tvlqr_periodic_steady_state_f64) beside the
way the same answer was had before it: the sequential Riccati recursion (tfmpc_tvlqr_backward_f64) over the horizon R N
of R tiled periods, on the same operands, in the same run.

    python tools/tvlqr_periodic_rate.py [--out profiles/tvlqr_periodic_rate.json] [--points 1x64 1x512 ...]
                                        [--max-segments 512] [--host-only]

n = 16, m = 8, tvlqr_ref.make_models operands (one period per N, drawn once and tiled over the batch with a relative 1e-9
perturbation per instance).  R is the smallest power of two at which the fp64 restatement of the tiled route (the
recursion in the kernel's Schur form from the default final cost, its first period kept) meets the budget rule of
tests/tvlqr_f64_ref.py against the longdouble periodic restatement with the fp64 periodic restatement's error as the
budget -- the accuracy the periodic kernel is held to; it is found on the host, on instance 0, and recorded per point.
Per (B, N): `segments` swept over powers of two from 1 up, every line and the tiled route timed with device events -- 40
untimed calls of every line, then 10 rounds that run the lines one after the other (alternating); median, minimum and
maximum per line, so that the run-to-run spread stands beside every ratio.  The phase split at the best `segments`: the
same call stopped after its condense, stitch and expand launch (TFMPC_TVLQR_TP_PHASES), differences of the medians.
--host-only finds R and stops (no GPU needed)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests")]

N_DIM, M_DIM = 16, 8
POINTS = ["1x64", "1x512", "1x4096", "64x512", "4096x50"]


def schur_backward(F, f, C, c, periods):
    """The fp64 recursion in the kernel's Schur form over `periods` tiled periods from the default final cost: the first
    period's dict(K, k, V, v)."""
    N, n = F.shape[0], F.shape[1]
    V, v = C[N - 1][:n, :n], c[N - 1][:n].reshape(n, 1)
    out = None
    for _ in range(periods):
        out = dict(K=[None] * N, k=[None] * N, V=[None] * N, v=[None] * N)
        for t in reversed(range(N)):
            Ft, ft, Ct, ct = F[t], f[t].reshape(n, 1), C[t], c[t].reshape(-1, 1)
            W = Ft.T @ V
            Q = Ct + W @ Ft
            q = ct + W @ ft + Ft.T @ v
            sol = -np.linalg.solve(Q[n:, n:], np.concatenate([q[n:], Q[n:, :n]], axis=1))
            k, K = sol[:, :1], sol[:, 1:]
            V = Q[:n, :n] + Q[:n, n:] @ K
            V, v = 0.5 * (V + V.T), q[:n] + Q[:n, n:] @ k
            out["K"][t], out["k"][t], out["V"][t], out["v"][t] = K, k[:, 0], V, v[:, 0]
    return {name: np.stack(a) for name, a in out.items()}


def sufficient_periods(F, f, C, c, segments, cap=4096):
    """(R, worst ratio at R, worst ratio at R / 2): the smallest power of two at which the tiled route meets the rule."""
    import tvlqr_f64_ref as ref64
    import tvlqr_periodic_ref as pr
    rld = pr.solve(F, f, C, c, segments, dtype=np.longdouble)
    r64 = pr.solve(F, f, C, c, segments)
    assert rld["status"] == 0 and r64["status"] == 0
    R, before = 1, None
    while R <= cap:
        got = schur_backward(F, f, C, c, R)
        worst = max(float(pr.ratios({name: [got[name]]}, [rld], [r64], name)[0]) for name in pr.FIELDS)
        if worst <= ref64.MEDIAN_BOUND:
            return R, worst, before
        R, before = 2 * R, worst
    raise RuntimeError(f"the tiled route does not meet the rule within {cap} periods")


def timed_alternating(fns, warm=40, reps=10):
    """{line: dict(median, min, max)} in ms."""
    import torch
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
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="+", default=POINTS, help="BxN")
    ap.add_argument("--max-segments", type=int, default=512)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import tvlqr_ref
    n, m = N_DIM, M_DIM
    points = []
    for spec in args.points:
        B, N = (int(x) for x in spec.split("x"))
        period = [a[0].astype(np.float64) for a in tvlqr_ref.make_models(n, m, N, 1, seed=N)]
        period[2] = 0.5 * (period[2] + np.swapaxes(period[2], -1, -2))
        R, ratio, ratio_before = sufficient_periods(*period, segments=max(1, int(round(N ** 0.5))))
        point = dict(B=B, N=N, tiled_periods=R, tiled_ratio=ratio, tiled_ratio_at_half=ratio_before)
        if args.host_only:
            print(json.dumps(point), flush=True)
            continue
        import torch
        from tfmpc import _hip
        from tfmpc.solvers import TimeVaryingLQR
        lib = _hip.require_gpu()
        dev = "cuda"
        base = [torch.as_tensor(a, device=dev) for a in period]
        gen = torch.Generator(device=dev).manual_seed(B)
        F, f, C, c = (a[None] * (1.0 + 1e-9 * torch.randn((B, *a.shape), generator=gen, device=dev, dtype=torch.float64)) for a in base)
        C = 0.5 * (C + C.transpose(-1, -2))
        tv = TimeVaryingLQR(F, f, C, c, device=dev, symmetric=True, dtype=torch.float64)
        tiled = TimeVaryingLQR(*(a.repeat(1, R, *([1] * (a.dim() - 2))) for a in (F, f, C, c)), device=dev, symmetric=True,
                               dtype=torch.float64)
        T = R * N
        K, k = torch.empty((B, T, m, n), device=dev, dtype=torch.float64), torch.empty((B, T, m), device=dev, dtype=torch.float64)
        V, v = torch.empty((B, T, n, n), device=dev, dtype=torch.float64), torch.empty((B, T, n), device=dev, dtype=torch.float64)
        residual = torch.empty(B, device=dev, dtype=torch.float64)
        iterations = torch.zeros(B, dtype=torch.int32, device=dev)
        status, status_tiled = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        sweep = [s for s in (2 ** i for i in range(0, 16)) if s <= min(N, args.max_segments)]
        need = max(int(lib.tfmpc_tvlqr_periodic_workspace_bytes_f64(B, n, m, N, s)) for s in sweep)
        ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=dev)
        model, model_tiled = tv._model_args(), tiled._model_args()

        def tiled_route():
            _hip.check(lib.tfmpc_tvlqr_backward_f64(B, n, m, T, *model_tiled, _hip.ptr(K), _hip.ptr(k), _hip.ptr(V), _hip.ptr(v), None,
                                                    _hip.ptr(status_tiled), _hip.stream()), "tfmpc_tvlqr_backward_f64")

        def periodic(segments, stopped=False):
            rc = lib.tfmpc_tvlqr_periodic_steady_state_f64(
                B, n, m, N, *model[:12], segments, 0, 0.0, _hip.ptr(K), _hip.ptr(k), _hip.ptr(V), _hip.ptr(v), _hip.ptr(residual),
                _hip.ptr(iterations), _hip.ptr(status), _hip.ptr(ws), ws.numel() * 8, _hip.stream())
            _hip.check(0 if stopped and rc == _hip.TVLQR_TP_STOPPED else rc, "tfmpc_tvlqr_periodic_steady_state_f64")

        lines = {"tiled": tiled_route}
        lines.update({f"segments_{s}": (lambda s=s: periodic(s)) for s in sweep})
        ms = timed_alternating(lines, warm=args.warm)
        torch.cuda.synchronize()
        best = min(sweep, key=lambda s: ms[f"segments_{s}"]["median"])
        periodic(best)
        torch.cuda.synchronize()
        flagged = int((status != 0).sum()) + int((status_tiled != 0).sum())
        doubling_steps = [int(iterations.min()), int(iterations.max())]
        worst_residual = float(residual.max())
        phases = {}
        for stop, name in (("1", "condense"), ("2", "condense_stitch"), ("3", "condense_stitch_expand")):
            with _hip.option("TFMPC_TVLQR_TP_PHASES", stop):
                phases[name] = timed_alternating({name: lambda: periodic(best, stopped=True)}, warm=args.warm)[name]["median"]
        full = ms[f"segments_{best}"]["median"]
        split = dict(condense=phases["condense"], stitch=phases["condense_stitch"] - phases["condense"],
                     expand=phases["condense_stitch_expand"] - phases["condense_stitch"],
                     finish=full - phases["condense_stitch_expand"])
        old, new = ms["tiled"], ms[f"segments_{best}"]
        point.update(ms=ms, best_segments=best, speedup=old["median"] / new["median"], speedup_worst_case=old["min"] / new["max"],
                     default_segments=tv.default_segments(B), phase_ms=split, flagged=flagged, doubling_steps=doubling_steps,
                     worst_residual=worst_residual)
        print(json.dumps(point), flush=True)
        points.append(point)
        del tiled, K, k, V, v, ws, F, f, C, c, tv
        torch.cuda.empty_cache()
    if args.host_only:
        return
    import torch
    from tfmpc import _hip
    lib = _hip.load()
    result = dict(n=n, m=m, device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count,
                  kernel=lib.tfmpc_tvlqr_periodic_kernel_name_f64(n, m, 512, 16).decode(),
                  tiled_kernel=lib.tfmpc_tvlqr_kernel_name_f64(n, m, 512).decode(), points=points,
                  method=f"device events, {args.warm} untimed calls per line, median (min, max) of 10 alternating rounds; tiled: "
                         "tfmpc_tvlqr_backward_f64 over tiled_periods x N steps, tiled_periods the smallest power of two at which the fp64 "
                         "restatement of that route meets the budget rule (ratio <= 2.5 on instance 0; tiled_ratio_at_half: the ratio one "
                         "power of two below); phase split: the call stopped after one, two and three launches, differences of medians")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
