"""Rate of the segmented adjoint of the time-parallel double-precision TV-LQR (tfmpc_tvlqr_vjp_time_parallel_f64,
DESIGN.md 3.24) beside the sequential VJP (tfmpc_tvlqr_vjp_f64) and the time-parallel forward
(tfmpc_tvlqr_solve_time_parallel_f64) of the same build on the same operands, in the same run.

    python tools/tvlqr_time_parallel_grad_rate.py [--out profiles/tvlqr_time_parallel_grad_rate.json] [--horizons 512 4096]
                                                  [--batches 1 8 64] [--max-segments 512]

n = 16, m = 8, tvlqr_ref.make_models operands (one model per horizon, drawn once and tiled over the batch with a relative
1e-9 perturbation per instance), mixed loss (g_states, g_actions, g_costs all given), every gradient per instance and per
step.  Per (T, B): `segments` swept over powers of two from 2 up for the forward and for the VJP, every line and the
sequential VJP timed with device events -- 40 untimed calls of every line, then 10 rounds that run the lines one after
the other (alternating); median, minimum and maximum per line, so that the run-to-run spread stands beside every ratio.
The phase split at the VJP's best `segments`: the same call stopped after each of its first six launches
(TFMPC_TVLQR_TP_PHASES), device events around it, differences of the medians."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402
from tvlqr_time_parallel_rate import timed_alternating  # noqa: E402

PHASES = ("fold_step", "condense", "stitch_back", "expand_back", "stitch_fwd", "expand_fwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizons", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--max-segments", type=int, default=512)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _hip.require_gpu()
    import tvlqr_ref
    n, m = 16, 8
    d = n + m
    dev, f64 = "cuda", torch.float64
    points = []
    for T in args.horizons:
        base = [torch.as_tensor(a[0].astype(np.float64), device=dev) for a in tvlqr_ref.make_models(n, m, T, 1, seed=T)]
        for B in args.batches:
            gen = torch.Generator(device=dev).manual_seed(B)
            F, f, C, c = (a[None] * (1.0 + 1e-9 * torch.randn((B, *a.shape), generator=gen, device=dev, dtype=f64)) for a in base)
            C = 0.5 * (C + C.transpose(-1, -2))
            tv = TimeVaryingLQR(F, f, C, c, device=dev, symmetric=True, dtype=f64)
            x0 = torch.randn((B, n, 1), generator=gen, device=dev, dtype=f64)
            fwd = tv._time_parallel_device(x0, None, True, True)
            states, actions, K, V, v = (fwd[k] for k in ("states", "actions", "K", "V", "v"))
            ups = [torch.randn(shape, generator=gen, device=dev, dtype=f64) for shape in ((B, T + 1, n), (B, T, m), (B, T + 1))]
            grads = [torch.empty(shape, device=dev, dtype=f64) for shape in ((B, T, n, d), (B, T, n), (B, T, d, d), (B, T, d), (B, n))]
            outs = []
            for g in grads[:4]:
                outs += [_hip.ptr(g), g[0].numel(), g[0, 0].numel()]
            outs += [None, 0, None, 0, _hip.ptr(grads[4]), n]
            status = torch.zeros(B, dtype=torch.int32, device=dev)
            scratch = [torch.empty_like(t) for t in (states, actions, fwd["costs"])]
            sweep = [s for s in (2 ** i for i in range(1, 16)) if s <= min(T, args.max_segments)]
            need = max([int(lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(B, n, m, T))]
                       + [int(lib.tfmpc_tvlqr_vjp_time_parallel_workspace_bytes_f64(B, n, m, T, s)) for s in sweep]
                       + [int(lib.tfmpc_tvlqr_time_parallel_workspace_bytes_f64(B, n, m, T, s)) for s in sweep])
            ws = torch.empty(need // 8 + 1, dtype=f64, device=dev)
            model = tv._model_args()
            given = [_hip.ptr(u) for u in ups]

            def sequential():
                _hip.check(lib.tfmpc_tvlqr_vjp_f64(B, n, m, T, *model, _hip.ptr(states), _hip.ptr(actions), _hip.ptr(v), *given, *outs,
                                                   _hip.ptr(status), _hip.ptr(ws), ws.numel() * 8, _hip.stream()), "tfmpc_tvlqr_vjp_f64")

            def segmented(segments, stopped=False):
                rc = lib.tfmpc_tvlqr_vjp_time_parallel_f64(B, n, m, T, *model, _hip.ptr(states), _hip.ptr(actions), _hip.ptr(v),
                                                           _hip.ptr(K), _hip.ptr(V), *given, *outs, _hip.ptr(status), segments,
                                                           _hip.ptr(ws), ws.numel() * 8, _hip.stream())
                _hip.check(0 if stopped and rc == _hip.TVLQR_TP_STOPPED else rc, "tfmpc_tvlqr_vjp_time_parallel_f64")

            def forward(segments):
                _hip.check(lib.tfmpc_tvlqr_solve_time_parallel_f64(
                    B, n, m, T, *model, _hip.ptr(x0), *(_hip.ptr(t) for t in scratch), None, None, None, None, None, _hip.ptr(status),
                    segments, _hip.ptr(ws), ws.numel() * 8, _hip.stream()), "tfmpc_tvlqr_solve_time_parallel_f64")

            lines = {"vjp_sequential": sequential}
            lines.update({f"vjp_segments_{s}": (lambda s=s: segmented(s)) for s in sweep})
            lines.update({f"forward_segments_{s}": (lambda s=s: forward(s)) for s in sweep})
            ms = timed_alternating(lines, warm=args.warm)
            segmented(sweep[0])
            torch.cuda.synchronize()
            flagged = int((status != 0).sum())
            best = min(sweep, key=lambda s: ms[f"vjp_segments_{s}"]["median"])
            best_fwd = min(sweep, key=lambda s: ms[f"forward_segments_{s}"]["median"])
            cum = {}
            for stop, name in enumerate(PHASES, start=1):
                with _hip.option("TFMPC_TVLQR_TP_PHASES", str(stop)):
                    cum[name] = timed_alternating({name: lambda: segmented(best, stopped=True)}, warm=args.warm)[name]["median"]
            full = ms[f"vjp_segments_{best}"]["median"]
            split, before = {}, 0.0
            for name in PHASES:
                split[name], before = cum[name] - before, cum[name]
            split["costates_and_sums"] = full - before
            seq, seg = ms["vjp_sequential"], ms[f"vjp_segments_{best}"]
            point = dict(T=T, B=B, ms=ms, best_segments=best, forward_best_segments=best_fwd, speedup=seq["median"] / seg["median"],
                         speedup_worst_case=seq["min"] / seg["max"],
                         backward_over_forward=ms[f"vjp_segments_{best_fwd}"]["median"] / ms[f"forward_segments_{best_fwd}"]["median"],
                         best_backward_over_best_forward=seg["median"] / ms[f"forward_segments_{best_fwd}"]["median"],
                         default_segments=tv.default_segments(B), default_vjp_segments=tv.default_vjp_segments(B), phase_ms=split,
                         flagged=flagged)
            print(json.dumps(point), flush=True)
            points.append(point)
    result = dict(n=n, m=m, device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count,
                  points=points,
                  method=f"device events, {args.warm} untimed calls per line, median (min, max) of 10 alternating rounds; mixed loss, every "
                         "gradient per instance and per step; phase split: the call stopped after one to six launches, differences of "
                         "medians")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
