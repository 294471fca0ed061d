"""Rate of the double-precision control-limited TV-LQR forward (tfmpc_tvlqr_box_solve_f64) beside the fp32
kernel of the same build (tfmpc_tvlqr_box_solve_f32) on the same problem, in the same run.

    python tools/tvlqr_box_solve_f64_rate.py [--batch 65536] [--out profiles/tvlqr_box_solve_f64_rate.json]

The method of tools/tvlqr_box_solve_rate.py: B x (n = 16, m = 8, T = 50), the numbers of workloads.control_limited_stable
(fp32 numbers, handed to the double kernel as doubles), the time-invariant model through stride-0 operands, device
events, 40 untimed calls of every line, then 10 timed rounds that run the lines one after the other (alternating); the
median per line.  Beside the times: the distribution of `iterations` (backward sweeps per instance), the status bits
and reasons of both kernels, and what the double kernel makes of the instances that profiles/tvlqr_box_solve_rate.json
lists as flagged by the fp32 kernel (`failed_instances`).  No time bar is set."""
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

BITS = dict(NOT_PD=2, NAN=4, QP_MAXITER=8, MAX_ATTEMPTS=16)


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
    lines = {}
    for name, dt, size, solve, query in (
            ("f32", torch.float32, 4, lib.tfmpc_tvlqr_box_solve_f32, lib.tfmpc_tvlqr_box_solve_workspace_bytes),
            ("f64", torch.float64, 8, lib.tfmpc_tvlqr_box_solve_f64, lib.tfmpc_tvlqr_box_solve_workspace_bytes_f64)):
        t = lambda a, dt=dt: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev).to(dt).contiguous()      # noqa: E731
        s = dict(model=[t(w[k]) for k in ("F", "f", "C", "c")], x0=w["x0"].reshape(B, n).to(dt).contiguous(),
                 low=torch.full((m,), -0.5, dtype=dt, device=dev), high=torch.full((m,), 0.5, dtype=dt, device=dev),
                 states=torch.empty(B, T + 1, n, dtype=dt, device=dev), actions=torch.empty(B, T, m, dtype=dt, device=dev),
                 costs=torch.empty(B, T + 1, dtype=dt, device=dev),
                 ws=torch.empty((query(B, n, m, T) + size - 1) // size, dtype=dt, device=dev), size=size, solve=solve, name=name)
        s["iterations"], s["status"], s["reason"] = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
        lines[name] = s

    def launch(s):
        model = []
        for a in s["model"]:
            model += [_hip.ptr(a), a[0].numel(), 0]
        rc = s["solve"](B, n, m, T, *model, None, 0, None, 0, _hip.ptr(s["low"]), 0, 0, _hip.ptr(s["high"]), 0, 0,
                        _hip.ptr(s["x0"]), None, 0, 0, 0.0, _hip.ptr(s["states"]), _hip.ptr(s["actions"]), _hip.ptr(s["costs"]),
                        _hip.ptr(s["iterations"]), _hip.ptr(s["status"]), _hip.ptr(s["reason"]), None, _hip.ptr(s["ws"]),
                        s["ws"].numel() * s["size"], _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_box_solve_" + s["name"])

    ms = timed_alternating({k: (lambda s=s: launch(s)) for k, s in lines.items()}, warm=args.warm)
    for s in lines.values():
        launch(s)
    torch.cuda.synchronize()

    def census(s):
        it, st, rs = (s[k].cpu().numpy() for k in ("iterations", "status", "reason"))
        return dict(iterations_histogram=np.bincount(it).tolist(), iterations_median=float(np.median(it)), iterations_max=int(it.max()),
                    flagged=int((st != 0).sum()), reasons=np.bincount(rs, minlength=4).tolist(), reason_1=int((rs == 1).sum()),
                    status_bits={k: int((st & v != 0).sum()) for k, v in BITS.items()},
                    failed_instances=np.nonzero(rs == 3)[0][:32].tolist())

    result = dict(B=B, n=n, m=m, T=T, workload=w["version"], kernel=lib.tfmpc_tvlqr_box_solve_kernel_name_f64(n, m, T).decode(),
                  fp32_kernel=lib.tfmpc_tvlqr_box_solve_kernel_name(n, m, T).decode(), ms=ms, ratio_f64_over_f32=ms["f64"] / ms["f32"],
                  f64=census(lines["f64"]), f32=census(lines["f32"]),
                  method=f"device events, {args.warm} untimed calls per line, median of 10 alternating rounds")
    # the instances the fp32 write-up lists as NOT_PD: what the double kernel makes of them
    listed = os.path.join(ROOT, "profiles", "tvlqr_box_solve_rate.json")
    if os.path.exists(listed) and B == json.load(open(listed))["B"]:
        d, f = lines["f64"], lines["f32"]
        x = d["states"]
        result["fp32_failed_instances_in_f64"] = [
            dict(instance=int(e["instance"]), fp32_status_listed=int(e["status"]), fp32_status=int(f["status"][e["instance"]]),
                 status=int(d["status"][e["instance"]]), reason=int(d["reason"][e["instance"]]),
                 iterations=int(d["iterations"][e["instance"]]), finite=bool(torch.isfinite(x[e["instance"]]).all()),
                 max_abs_state=float(x[e["instance"]].abs().max()))
            for e in json.load(open(listed))["failed_instances"]]
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
