"""Rate of the time-parallel double-precision TV-LQR solve (tfmpc_tvlqr_solve_time_parallel_f64) beside
the sequential kernel of the same build (tfmpc_tvlqr_solve_f64) on the same operands, in the same run.

    python tools/tvlqr_time_parallel_rate.py [--out profiles/tvlqr_time_parallel_rate.json] [--horizons 512 4096]
                                             [--batches 1 8 64 1024] [--max-segments 512]

n = 16, m = 8, tvlqr_ref.make_models operands (one model per horizon, drawn once and tiled over the batch with a relative
1e-9 perturbation per instance).  Per (T, B): `segments` swept over powers of two from 2 up, every line and the
sequential solve timed with device events -- 40 untimed calls of every line, then 10 rounds that run the lines one after
the other (alternating); median, minimum and maximum per line, so that the run-to-run spread stands beside every ratio.
The phase split at the best `segments`: the same call stopped after its condense and after its stitch launch
(TFMPC_TVLQR_TP_PHASES), device events around it, differences of the medians."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tf-mpc_amd"), os.path.join(ROOT, "tests")]
from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402


def timed_alternating(fns, warm=40, reps=10):
    """{line: dict(median, min, max)} in ms."""
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
    ap.add_argument("--horizons", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 1024])
    ap.add_argument("--max-segments", type=int, default=512)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _hip.require_gpu()
    import tvlqr_ref
    n, m = 16, 8
    dev = "cuda"
    points = []
    for T in args.horizons:
        base = [torch.as_tensor(a[0].astype(np.float64), device=dev) for a in tvlqr_ref.make_models(n, m, T, 1, seed=T)]
        for B in args.batches:
            gen = torch.Generator(device=dev).manual_seed(B)
            F, f, C, c = (a[None] * (1.0 + 1e-9 * torch.randn((B, *a.shape), generator=gen, device=dev, dtype=torch.float64)) for a in base)
            C = 0.5 * (C + C.transpose(-1, -2))
            tv = TimeVaryingLQR(F, f, C, c, device=dev, symmetric=True, dtype=torch.float64)
            x0 = torch.randn((B, n, 1), generator=gen, device=dev, dtype=torch.float64)
            states, actions, costs = (torch.empty((B, T + 1, n), device=dev, dtype=torch.float64),
                                      torch.empty((B, T, m), device=dev, dtype=torch.float64),
                                      torch.empty((B, T + 1), device=dev, dtype=torch.float64))
            status = torch.zeros(B, dtype=torch.int32, device=dev)
            sweep = [s for s in (2 ** i for i in range(1, 16)) if s <= min(T, args.max_segments)]
            need = max(int(lib.tfmpc_tvlqr_time_parallel_workspace_bytes_f64(B, n, m, T, s)) for s in sweep)
            ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=dev)
            model = tv._model_args()

            def sequential():
                _hip.check(lib.tfmpc_tvlqr_solve_f64(B, n, m, T, *model, _hip.ptr(x0), _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs),
                                                     None, None, None, None, None, _hip.ptr(status), _hip.ptr(ws), ws.numel() * 8,
                                                     _hip.stream()), "tfmpc_tvlqr_solve_f64")

            def parallel(segments, stopped=False):
                rc = lib.tfmpc_tvlqr_solve_time_parallel_f64(
                    B, n, m, T, *model, _hip.ptr(x0), _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs), None, None, None, None, None,
                    _hip.ptr(status), segments, _hip.ptr(ws), ws.numel() * 8, _hip.stream())
                _hip.check(0 if stopped and rc == _hip.TVLQR_TP_STOPPED else rc, "tfmpc_tvlqr_solve_time_parallel_f64")

            lines = {"sequential": sequential}
            lines.update({f"segments_{s}": (lambda s=s: parallel(s)) for s in sweep})
            ms = timed_alternating(lines, warm=args.warm)
            torch.cuda.synchronize()
            flagged = int((status != 0).sum())
            best = min(sweep, key=lambda s: ms[f"segments_{s}"]["median"])
            phases = {}
            for stop, name in (("1", "condense"), ("2", "condense_stitch")):
                with _hip.option("TFMPC_TVLQR_TP_PHASES", stop):
                    phases[name] = timed_alternating({name: lambda: parallel(best, stopped=True)}, warm=args.warm)[name]["median"]
            full = ms[f"segments_{best}"]["median"]
            split = dict(condense=phases["condense"], stitch=phases["condense_stitch"] - phases["condense"],
                         expand_and_finish=full - phases["condense_stitch"])
            seq, par = ms["sequential"], ms[f"segments_{best}"]
            point = dict(T=T, B=B, ms=ms, best_segments=best, speedup=seq["median"] / par["median"],
                         speedup_worst_case=seq["min"] / par["max"], default_segments=tv.default_segments(B), phase_ms=split,
                         flagged=flagged)
            print(json.dumps(point), flush=True)
            points.append(point)
    result = dict(n=n, m=m, device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count,
                  kernel=lib.tfmpc_tvlqr_time_parallel_kernel_name_f64(n, m, 4096, 64).decode(),
                  sequential_kernel=lib.tfmpc_tvlqr_kernel_name_f64(n, m, 4096).decode(), points=points,
                  method=f"device events, {args.warm} untimed calls per line, median (min, max) of 10 alternating rounds; phase split: the call "
                         "stopped after one and two launches, differences of medians")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
