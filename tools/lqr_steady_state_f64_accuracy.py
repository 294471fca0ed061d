"""Measured accuracy of the double-precision infinite-horizon LQR (tfmpc_lqr_steady_state_f64) against
the 80-bit restatement of tests/lqr_steady_state_f64_ref.py, on the operands of tests/test_lqr_steady_state_f64_gpu.py
(B = 6 per shape, both workloads):

  per shape and output: the largest error relative to the output's scale, and the budget rule's ratio (median / max);
  at (16, 8), per output: the fp32 kernel's error over the double kernel's (floored at 2^-48 of the scale), per instance.

Prints one JSON object.  Usage: python tools/lqr_steady_state_f64_accuracy.py [--out file.json]"""
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

import lqr_steady_state_f64_ref as ref64  # noqa: E402
from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import lqr_steady_state  # noqa: E402
from tfmpc.solvers.lqr import LQR  # noqa: E402

SHAPES = [(1, 1), (3, 2), (12, 6), (16, 8), (16, 16), (17, 8), (16, 17), (22, 3), (32, 16), (32, 32)]


def host(ss):
    got = {name: getattr(ss, name).cpu().numpy() for name in ref64.FIELDS + ("iterations", "status")}
    got["k"], got["p"] = got["k"][..., 0], got["p"][..., 0]
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    _hip.require_gpu()
    out = {"B": 6, "device": torch.cuda.get_device_name(0), "shapes": [], "fp32_error_over_fp64_error_16x8": {}}
    for kind in ("make_lqr", "damped"):
        for n, m in SHAPES:
            ops = ref64.operands(kind, n, m, 6, seed=10 * n + m)
            refs = ref64.references(*ops)
            got = host(lqr_steady_state(*ops, dtype=torch.float64))
            row = {"workload": kind, "n": n, "m": m, "kernel": _hip.load().tfmpc_lqr_steady_state_kernel_name_f64(n, m).decode(),
                   "flagged": int((got["status"] != 0).sum()), "iterations_max": int(got["iterations"].max()),
                   "iterations_fp64_restatement_max": max(r["iterations"] for r in refs[1])}
            for name in ref64.FIELDS:
                r = ref64.ratios(got, refs, name)
                rel = [ref64.error(got[name][b], ld[name]) / ref64.scale_of(ld[name]) for b, ld in enumerate(refs[0])]
                row[name] = {"rel_error_max": max(rel), "budget_ratio_median": float(np.median(r)), "budget_ratio_max": float(r.max())}
            out["shapes"].append(row)
            if (n, m) == (16, 8):
                got32 = host(LQR(*ops, device="cuda").steady_state())
                gains = {}
                for name in ref64.FIELDS:
                    g = []
                    for b, ld in enumerate(refs[0]):
                        e64 = max(ref64.error(got[name][b], ld[name]), ref64.FLOOR * ref64.scale_of(ld[name]))
                        g.append(ref64.error(got32[name][b], ld[name]) / e64)
                    gains[name] = {"min": min(g), "median": float(np.median(g))}
                out["fp32_error_over_fp64_error_16x8"][kind] = gains
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
