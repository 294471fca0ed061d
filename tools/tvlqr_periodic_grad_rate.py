"""Rate of the gradients of the periodic infinite-horizon LQR in double (tfmpc_tvlqr_periodic_vjp_f64)
beside the only other way to those gradients: tfmpc_tvlqr_backward_vjp_f64 over R tiled periods with the upstream
gradients on the first tile, plus the sum over the tiles.

    python tools/tvlqr_periodic_grad_rate.py [--out profiles/tvlqr_periodic_grad_rate.json] [--points 1x64 1x512 ...]

n = 16, m = 8, tests/tvlqr_ref.py make_models operands (one period, repeated over the batch with a 1e-9 relative
perturbation), all four upstream gradients, gradients per instance and per step.  R is the smallest power of two at which
the fp64 restatement of the tiled route (tests/tvlqr_backward_grad_f64_ref.py closed_form from its own fp64 recursion,
the tiles' gradients added) meets the rule the kernel is held to: worst ratio over dF, df, dC, dc <= 2.5 against the
longdouble restatement with the fp64 restatement's error as the budget; it is found on the host, on instance 0, and
recorded per point (--tiled-periods gives it instead: one value per point, found by an earlier --host-only run).
Method: tools/tvlqr_periodic_rate.py's -- device events, 40 untimed calls of every line, then 10 alternating rounds;
median, minimum and maximum per line.  The tiled line times the VJP over R N steps and the sum over the tiles (the tiled
forward it also needs is timed on a line of its own, and not counted).  The phase split at the best `segments`: the call
stopped after each of its first five launches (TFMPC_TVLQR_TP_PHASES), differences of the medians."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from tvlqr_periodic_rate import M_DIM, N_DIM, POINTS, timed_alternating      # noqa: E402

PHASES = ("pass_a", "stitch_a", "pass_b", "stitch_b", "pass_c")


def sufficient_periods(period, ups, segments, cap=1024):
    """(R, worst ratio at R, worst ratio at R / 2) for one instance: operands [N, ...], ups name -> [N, ...]."""
    import tvlqr_backward_grad_f64_ref as gr64
    import tvlqr_periodic_grad_ref as pg
    import tvlqr_periodic_ref as pr
    one = [a[None] for a in period]
    up1 = {k: g[None] for k, g in ups.items()}
    refs = pg.references(*one, up1, segments, pr.solve_batch(*one, segments, dtype=np.longdouble), pr.solve_batch(*one, segments))
    N = period[0].shape[0]
    R, before = 1, None
    while R <= cap:
        tile = lambda a: np.concatenate([a] * R, axis=1)                  # noqa: E731
        pad = lambda g: np.concatenate([g, np.zeros((1, (R - 1) * N) + g.shape[2:])], axis=1)      # noqa: E731
        r = gr64.closed_form(*(tile(a) for a in one), **{k: pad(g) for k, g in up1.items()})
        got = {name: r[name].reshape(1, R, N, *r[name].shape[2:]).sum(axis=1) for name in pg.GRADS}
        worst = max(float(gr64.ratios(got[name], refs, name)[0]) for name in pg.GRADS)
        if worst <= gr64.MEDIAN_BOUND:
            return R, worst, before
        R, before = 2 * R, worst
    raise RuntimeError(f"the tiled route does not meet the rule within {cap} periods")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="+", default=POINTS, help="BxN")
    ap.add_argument("--tiled-periods", nargs="+", type=int, default=None, help="R per point, from a --host-only run")
    ap.add_argument("--max-segments", type=int, default=512)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import tvlqr_periodic_grad_ref as pg
    import tvlqr_ref
    n, m = N_DIM, M_DIM
    points = []
    for i, spec in enumerate(args.points):
        B, N = (int(x) for x in spec.split("x"))
        period = [a[0].astype(np.float64) for a in tvlqr_ref.make_models(n, m, N, 1, seed=N)]
        period[2] = 0.5 * (period[2] + np.swapaxes(period[2], -1, -2))
        ups1 = {k: g[0] for k, g in pg.upstream(n, m, N, 1, seed=N).items()}
        if args.tiled_periods:
            point = dict(B=B, N=N, tiled_periods=args.tiled_periods[i], tiled_periods_from="an earlier --host-only run")
        else:
            R, ratio, ratio_before = sufficient_periods(period, ups1, max(1, int(round(N ** 0.5))))
            point = dict(B=B, N=N, tiled_periods=R, tiled_ratio=ratio, tiled_ratio_at_half=ratio_before)
        if args.host_only:
            print(json.dumps(point), flush=True)
            continue
        R = point["tiled_periods"]
        import torch
        from tfmpc import _hip
        from tfmpc.solvers import TimeVaryingLQR
        lib = _hip.require_gpu()
        dev, f64 = "cuda", torch.float64
        gen = torch.Generator(device=dev).manual_seed(B)
        F, f, C, c = (torch.as_tensor(a, device=dev)[None] * (1.0 + 1e-9 * torch.randn((B, *a.shape), generator=gen, device=dev, dtype=f64))
                      for a in period)
        C = 0.5 * (C + C.transpose(-1, -2))
        tv = TimeVaryingLQR(F, f, C, c, device=dev, symmetric=True, dtype=f64)
        tiled = TimeVaryingLQR(*(a.repeat(1, R, *([1] * (a.dim() - 2))) for a in (F, f, C, c)), device=dev, symmetric=True, dtype=f64)
        T, d = R * N, n + m
        up = [torch.as_tensor(ups1[k], device=dev)[None].repeat(B, *([1] * ups1[k].ndim)).contiguous() for k in pg.UPS]
        up_tiled = [torch.cat([g, torch.zeros((B, T - N, *g.shape[2:]), device=dev, dtype=f64)], dim=1).contiguous() for g in up]
        fwd = tv._periodic_launch(tv.default_segments(B), 0, 0.0)
        fwd_t = tiled._backward_launch()
        sizes = ((n, d), (n,), (d, d), (d,))
        grads = [torch.empty((B, N, *s), device=dev, dtype=f64) for s in sizes]
        grads_t = [torch.empty((B, T, *s), device=dev, dtype=f64) for s in sizes]
        sums_t = [torch.empty((B, N, *s), device=dev, dtype=f64) for s in sizes]
        residual = torch.empty(B, device=dev, dtype=f64)
        iterations, status, status_t = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
        sweep = [s for s in (2 ** i for i in range(0, 16)) if s <= min(N, args.max_segments)]
        need = max(int(lib.tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(B, n, m, N, s)) for s in sweep)
        ws = torch.empty(need // 8 + 1, dtype=f64, device=dev)
        need_f = max(int(lib.tfmpc_tvlqr_periodic_workspace_bytes_f64(B, n, m, N, s)) for s in sweep)
        ws_f = torch.empty(need_f // 8 + 1, dtype=f64, device=dev)
        model, model_tiled = tv._model_args()[:12], tiled._model_args()

        def strided(gs, steps):
            out = []
            for g in gs:
                out += [_hip.ptr(g), g[0].numel(), g[0, 0].numel()]
            return out

        def tiled_route():
            _hip.check(lib.tfmpc_tvlqr_backward_vjp_f64(
                B, n, m, T, *model_tiled, *(_hip.ptr(t) for t in fwd_t[:4]), _hip.ptr(fwd_t[5]), *(_hip.ptr(u) for u in up_tiled), None,
                *strided(grads_t, T), None, 0, None, 0, _hip.ptr(status_t), None, 0, _hip.stream()), "tfmpc_tvlqr_backward_vjp_f64")
            for s, g in zip(sums_t, grads_t):
                torch.sum(g.view(B, R, N, *g.shape[2:]), dim=1, out=s)

        def tiled_forward():
            tiled._backward_launch()

        def periodic(segments, stopped=False):
            rc = lib.tfmpc_tvlqr_periodic_vjp_f64(
                B, n, m, N, *model, *(_hip.ptr(t) for t in fwd[:4]), _hip.ptr(fwd[6]), *(_hip.ptr(u) for u in up), *strided(grads, N),
                _hip.ptr(residual), _hip.ptr(iterations), _hip.ptr(status), segments, 0, 0.0, _hip.ptr(ws), ws.numel() * 8, _hip.stream())
            _hip.check(0 if stopped and rc == _hip.TVLQR_TP_STOPPED else rc, "tfmpc_tvlqr_periodic_vjp_f64")

        def forward(segments):
            _hip.check(lib.tfmpc_tvlqr_periodic_steady_state_f64(
                B, n, m, N, *model, segments, 0, 0.0, *(_hip.ptr(t) for t in fwd[:7]), _hip.ptr(ws_f), ws_f.numel() * 8, _hip.stream()),
                "tfmpc_tvlqr_periodic_steady_state_f64")

        lines = {"tiled": tiled_route, "tiled_forward": tiled_forward}
        lines.update({f"segments_{s}": (lambda s=s: periodic(s)) for s in sweep})
        lines.update({f"forward_segments_{s}": (lambda s=s: forward(s)) for s in sweep})
        ms = timed_alternating(lines, warm=args.warm)
        torch.cuda.synchronize()
        best = min(sweep, key=lambda s: ms[f"segments_{s}"]["median"])
        best_f = min(sweep, key=lambda s: ms[f"forward_segments_{s}"]["median"])
        periodic(best)
        tiled_route()
        torch.cuda.synchronize()
        flagged = int((status != 0).sum()) + int((status_t != 0).sum())
        agree = max(float((a - b).abs().max() / max(1.0, float(a.abs().max()))) for a, b in zip(grads, sums_t))
        stops = {}
        for stop, name in enumerate(PHASES, 1):
            with _hip.option("TFMPC_TVLQR_TP_PHASES", str(stop)):
                stops[name] = timed_alternating({name: lambda: periodic(best, stopped=True)}, warm=args.warm)[name]["median"]
        full = ms[f"segments_{best}"]["median"]
        edges = [0.0] + [stops[name] for name in PHASES] + [full]
        split = dict(zip(PHASES + ("finish",), (b - a for a, b in zip(edges, edges[1:]))))
        old, new = ms["tiled"], ms[f"segments_{best}"]
        point.update(ms=ms, best_segments=best, speedup=old["median"] / new["median"], speedup_worst_case=old["min"] / new["max"],
                     speedup_at_one_segment=old["median"] / ms["segments_1"]["median"],
                     best_forward_segments=best_f, ratio_to_forward=new["median"] / ms[f"forward_segments_{best_f}"]["median"],
                     default_segments=tv.default_periodic_vjp_segments(B), phase_ms=split, flagged=flagged,
                     smith_steps=[int(iterations.min()), int(iterations.max())], worst_residual=float(residual.max()),
                     tiled_route_agrees_to=agree)
        print(json.dumps(point), flush=True)
        points.append(point)
        del tiled, grads_t, sums_t, up_tiled, fwd_t, ws, F, f, C, c, tv
        torch.cuda.empty_cache()
    if args.host_only:
        return
    import torch
    from tfmpc import _hip
    lib = _hip.load()
    result = dict(n=n, m=m, device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count,
                  kernel=lib.tfmpc_tvlqr_periodic_vjp_kernel_name_f64(n, m, 512, 16).decode(),
                  tiled_kernel=lib.tfmpc_tvlqr_backward_vjp_kernel_name_f64(n, m, 512).decode(), points=points,
                  method=f"device events, {args.warm} untimed calls per line, median (min, max) of 10 alternating rounds; tiled: "
                         "tfmpc_tvlqr_backward_vjp_f64 over tiled_periods x N steps with the upstream gradients on the first tile, plus "
                         "the sum over the tiles (the tiled forward is a line of its own, not counted); tiled_periods: the smallest "
                         "power of two at which the fp64 restatement of that route meets the budget rule (ratio <= 2.5 on instance 0); "
                         "phase split: the call stopped after each of its first five launches, differences of medians",
                  not_measured=["hardware counters", "the rate of the <32> instantiation (n or m above 16)"])
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
