"""Device-event times of the steady state's gradients (tfmpc_lqr_steady_state_vjp_f32) against its forward
(tfmpc_lqr_steady_state_f32) at B = 65 536, n = 16, m = 8, upstream gradients on all of K, k, P, p:

  (a) make_lqr(16, 8) draws, every operand per instance;
  (b) the lightly damped workload (closed-loop radius ~0.997), every operand per instance;
  (c) F, f and C shared by the batch, c per instance (goals): dF, df, dC summed over the batch.  The same call with
      those three written per instance instead gives the cost of the batch reduction (records + two-stage sums);
  (d) for scale, autograd through a batched fp32 torch restatement of the doubling (torch.linalg.solve, the same
      number of doubling steps as the kernel's median) on the same device, on line (a)'s problems.

Instances are a pool of 512 distinct draws, instance b holding its own copy of pool[b % 512].  Kernel times are the
ABI calls with preallocated buffers.  Prints one JSON object (median / min of --reps timed calls after --warmup).

--dtype float64 times the double gradients (tfmpc_lqr_steady_state_vjp_f64) on lines (a), (b), (c), the
same numbers upcast: the double VJP, the fp32 VJP and the double forward take turns in one process, one timed call each
per round, --reps rounds after --warmup; the whole measurement runs twice, and the gap between the two medians is the
spread a ratio of this file can be trusted to.  Writes the JSON line to --out (default
profiles/lqr_steady_state_grad_f64_rate.json).
Usage: python tools/lqr_steady_state_grad_rate.py [--dtype float64] [--reps 20] [--warmup 3] [--out file.json]"""
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

import lqr_steady_state_ref as ssref  # noqa: E402
from tfmpc import _hip  # noqa: E402
from tfmpc.solvers.lqr import LQR, _steady_state_launch_f64  # noqa: E402

B, N, M, POOL = 65536, 16, 8, 512


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


class Vjp:
    """Preallocated buffers of one tfmpc_lqr_steady_state_vjp_f32 call; `summed` names the outputs summed over the batch."""

    def __init__(self, lqr, ss, summed=()):
        self.lib = _hip.load()
        self.lqr, self.ss = lqr, ss
        n, m, d = N, M, N + M
        g = torch.Generator(device="cuda").manual_seed(0)
        self.up = [torch.randn(s, device="cuda", generator=g) for s in ((B, m, n), (B, m), (B, n, n), (B, n))]
        sizes = dict(F=n * d, f=n, C=d * d, c=d)
        self.outs = []
        for name in ("F", "f", "C", "c"):
            t = torch.empty((sizes[name] if name in summed else B * sizes[name],), device="cuda")
            self.outs += [t, 0 if name in summed else sizes[name]]
        self.ws_bytes = int(self.lib.tfmpc_lqr_steady_state_vjp_workspace_bytes(B, n, m)) if summed else 0
        self.ws = torch.empty(((self.ws_bytes + 3) // 4,), device="cuda") if summed else None
        self.status = torch.empty((B,), dtype=torch.int32, device="cuda")

    def __call__(self):
        lqr, ss = self.lqr, self.ss
        model = []
        for t in (lqr.F, lqr.f, lqr.C, lqr.c):
            model += [_hip.ptr(t), t.stride(0) if t.dim() == 3 else 0]
        outs = [(_hip.ptr(x) if i % 2 == 0 else x) for i, x in enumerate(self.outs)]
        rc = self.lib.tfmpc_lqr_steady_state_vjp_f32(B, N, M, *model, *(_hip.ptr(t) for t in ss[:4]), _hip.ptr(ss[5]),
                                                     *(_hip.ptr(u) for u in self.up), 0, 0.0, *outs, _hip.ptr(self.status),
                                                     _hip.ptr(self.ws), self.ws_bytes, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_steady_state_vjp_f32")


class Vjp64:
    """Preallocated buffers of one tfmpc_lqr_steady_state_vjp_f64 call on the double `model` (F, f, C, c) and its forward `ss`."""

    def __init__(self, model, ss, up, summed=()):
        self.lib = _hip.load()
        self.model, self.ss = model, ss
        n, m, d = N, M, N + M
        self.up = [u.double() for u in up]
        sizes = dict(F=n * d, f=n, C=d * d, c=d)
        self.outs = []
        for name in ("F", "f", "C", "c"):
            t = torch.empty((sizes[name] if name in summed else B * sizes[name],), device="cuda", dtype=torch.float64)
            self.outs += [t, 0 if name in summed else sizes[name]]
        self.ws_bytes = int(self.lib.tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(B, n, m)) if summed else 0
        self.ws = torch.empty(((self.ws_bytes + 7) // 8,), device="cuda", dtype=torch.float64) if summed else None
        self.status = torch.empty((B,), dtype=torch.int32, device="cuda")

    def __call__(self):
        model = []
        for t in self.model:
            model += [_hip.ptr(t), t.stride(0) if t.dim() == 3 else 0]
        outs = [(_hip.ptr(x) if i % 2 == 0 else x) for i, x in enumerate(self.outs)]
        rc = self.lib.tfmpc_lqr_steady_state_vjp_f64(B, N, M, *model, *(_hip.ptr(t) for t in self.ss[:4]), _hip.ptr(self.ss[5]),
                                                     *(_hip.ptr(u) for u in self.up), 0, 0.0, *outs, _hip.ptr(self.status),
                                                     _hip.ptr(self.ws), self.ws_bytes, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_steady_state_vjp_f64")


def taking_turns(fns, reps, warmup):
    """name -> median ms of `reps` timed calls, the functions called one after the other in every round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: float(np.median(v)) for name, v in ts.items()}


def line_f64(name, lqr, reps, warmup, summed=()):
    ss32 = lqr._steady_state_launch(0, 0.0)
    model = [t.double().contiguous() for t in (lqr.F, lqr.f, lqr.C, lqr.c)]
    forward = lambda: _steady_state_launch_f64(*model, lqr.batch_size, 0, 0.0)      # noqa: E731
    ss64 = forward()
    v32 = Vjp(lqr, ss32, summed)
    v64 = Vjp64(model, ss64, v32.up, summed)
    v64()
    torch.cuda.synchronize()
    fns = {"vjp_f64": v64, "vjp_f32": v32, "forward_f64": forward}
    first, second = taking_turns(fns, reps, warmup), taking_turns(fns, reps, warmup)
    out = {f"{name}_flagged": int((ss64[5] != 0).sum()), f"{name}_backward_flagged": int((v64.status != 0).sum())}
    for key in fns:
        out[f"{name}_{key}_ms"] = first[key]
        out[f"{name}_{key}_repeat_ms"] = second[key]
        out[f"{name}_{key}_spread"] = abs(first[key] - second[key]) / min(first[key], second[key])
    out[f"{name}_backward_over_forward_f64"] = first["vjp_f64"] / first["forward_f64"]
    out[f"{name}_vjp_f64_over_vjp_f32"] = first["vjp_f64"] / first["vjp_f32"]
    return out


def line(name, lqr, reps, warmup, summed=()):
    ss = lqr._steady_state_launch(0, 0.0)
    torch.cuda.synchronize()
    fwd_flagged = int((ss[5] != 0).sum())
    fmed, fmin = timed(lambda: lqr._steady_state_launch(0, 0.0), reps, warmup)
    vjp = Vjp(lqr, ss, summed)
    vjp()
    torch.cuda.synchronize()
    out = {f"{name}_forward_ms": fmed, f"{name}_forward_min_ms": fmin, f"{name}_flagged": fwd_flagged,
           f"{name}_backward_flagged": int((vjp.status != 0).sum()),
           f"{name}_forward_iterations_median": float(ss[4].float().median())}
    bmed, bmin = timed(vjp, reps, warmup)
    out.update({f"{name}_backward_ms": bmed, f"{name}_backward_min_ms": bmin, f"{name}_backward_over_forward": bmed / fmed})
    if summed:
        per = Vjp(lqr, ss, ())
        pmed, _ = timed(per, reps, warmup)
        out.update({f"{name}_backward_per_instance_outputs_ms": pmed, f"{name}_reduction_ms": bmed - pmed,
                    f"{name}_reduction_share": (bmed - pmed) / bmed})
    return out


def torch_doubling(F, f, C, c, iters):
    """Batched fp32 torch restatement of lqr_steady_state_ref.steady_state (fixed doubling count, no checks)."""
    n = F.shape[-2]
    A, Bm = F[..., :n], F[..., n:]
    Q, S, R = C[..., :n, :n], C[..., :n, n:], C[..., n:, n:]
    cx, cu = c[..., :n, :], c[..., n:, :]
    T = lambda X: X.transpose(-1, -2)          # noqa: E731
    sym = lambda X: 0.5 * (X + T(X))           # noqa: E731
    X = torch.linalg.solve(R, torch.cat([T(S), T(Bm)], -1))
    Ak, G, H = A - Bm @ X[..., :n], sym(Bm @ X[..., n:]), sym(Q - S @ X[..., :n])
    eye = torch.eye(n, device=F.device).expand_as(Ak)
    for _ in range(iters):
        Y = torch.linalg.solve(eye + G @ H, torch.cat([Ak, G], -1))
        Y1, Y2 = Y[..., :n], Y[..., n:]
        G = G + sym(Ak @ Y2 @ T(Ak))
        H = H + sym(T(Ak) @ H @ Y1)
        Ak = Ak @ Y1
    P = H
    Muu = sym(R + T(Bm) @ P @ Bm)
    K = -torch.linalg.solve(Muu, T(Bm) @ P @ A + T(S))
    Acl = A + Bm @ K
    p = torch.linalg.solve(eye - T(Acl), cx + T(K) @ cu + T(Acl) @ P @ f)
    k = -torch.linalg.solve(Muu, cu + T(Bm) @ (P @ f + p))
    return K, k, P, p


def torch_line(pool, iters, reps):
    idx = np.arange(B) % POOL
    ops = [torch.as_tensor(a[idx], device="cuda") for a in pool]
    ops[1], ops[3] = ops[1][..., None], ops[3][..., None]
    g = torch.Generator(device="cuda").manual_seed(0)
    ups = [torch.randn(s, device="cuda", generator=g) for s in ((B, M, N), (B, M, 1), (B, N, N), (B, N, 1))]

    def once():
        leaves = [t.detach().requires_grad_() for t in ops]
        outs = torch_doubling(*leaves, iters)
        loss = sum((u * o).sum() for u, o in zip(ups, outs))
        return loss, leaves

    def fwd():
        with torch.no_grad():
            torch_doubling(*ops, iters)

    fmed, _ = timed(fwd, max(3, reps // 4), 1)
    ts = []
    for _ in range(max(3, reps // 4)):
        loss, _ = once()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"d_torch_autograd_iterations": iters, "d_torch_forward_ms": fmed, "d_torch_backward_ms": float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    args = ap.parse_args()
    _hip.require_gpu()
    torch.cuda.set_device(0)
    idx = np.arange(B) % POOL
    a = ssref.make_lqr_batch(N, M, POOL, seed=0)
    d = ssref.damped_workload(N, M, POOL, seed=0)
    if args.dtype == "float64":
        lib = _hip.load()
        out = {"B": B, "n": N, "m": M, "kernel": lib.tfmpc_lqr_steady_state_vjp_kernel_name_f64(N, M).decode(),
               "kernel_f32": lib.tfmpc_lqr_steady_state_vjp_kernel_name(N, M).decode(),
               "forward_kernel": lib.tfmpc_lqr_steady_state_kernel_name_f64(N, M).decode(), "reps": args.reps,
               "warmup": args.warmup, "order": "vjp_f64, vjp_f32, forward_f64 take turns; two runs of reps rounds"}
        out.update(line_f64("a_make_lqr", LQR(*(x[idx] for x in a), device="cuda", symmetric=True), args.reps, args.warmup))
        out.update(line_f64("b_damped", LQR(*(x[idx] for x in d), device="cuda", symmetric=True), args.reps, args.warmup))
        goals = np.random.default_rng(1).normal(size=(B, N + M)).astype(np.float32)
        shared = LQR(a[0][0], a[1][0], a[2][0], goals, device="cuda", symmetric=True)
        out.update(line_f64("c_shared", shared, args.reps, args.warmup, summed=("F", "f", "C")))
        text = json.dumps(out)
        print(text)
        with open(args.out or os.path.join(ROOT, "profiles", "lqr_steady_state_grad_f64_rate.json"), "w") as fh:
            fh.write(text + "\n")
        return
    out = {"B": B, "n": N, "m": M, "kernel": _hip.load().tfmpc_lqr_steady_state_vjp_kernel_name(N, M).decode(), "reps": args.reps}
    out.update(line("a_make_lqr", LQR(*(x[idx] for x in a), device="cuda", symmetric=True), args.reps, args.warmup))
    out.update(line("b_damped", LQR(*(x[idx] for x in d), device="cuda", symmetric=True), args.reps, args.warmup))
    goals = np.random.default_rng(1).normal(size=(B, N + M)).astype(np.float32)
    shared = LQR(a[0][0], a[1][0], a[2][0], goals, device="cuda", symmetric=True)
    out.update(line("c_shared", shared, args.reps, args.warmup, summed=("F", "f", "C")))
    iters = int(round(out["a_make_lqr_forward_iterations_median"]))
    out.update(torch_line(a, iters, args.reps))
    out["d_torch_backward_over_kernel_backward"] = out["d_torch_backward_ms"] / out["a_make_lqr_backward_ms"]
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
