"""TEST INFRASTRUCTURE ONLY -- shapes, instances and launch helpers of the wide-shape tests of the shape-generic LQR
kernels (lqr_generic.hip, lqr_block.hip, tvlqr_generic.hip over wave_ops.h / block_ops.h): n + m > 64, n > 64, m > 64,
the thin edges, the largest shape one wave's LDS holds, and cost matrices whose pivoted elimination exchanges rows.

* ``SHAPES``: (n, m, T) of the table; ``boundary_n(lib, m)`` finds the largest supported n at run time.
* ``case(n, m, T)``: five instances of ``problems.make_lqr_batch_spd`` (F scaled to a spectral radius ~1.5) and their fp64 /
  fp32 oracle solves, made once and read-only.
* ``exchanges(Q_uu)`` / ``exchange_counts(problem, V64)``: how many rows a partial-pivot Gauss-Jordan elimination (first
  row of maximal |entry|, the kernels' rule) exchanges on the fp64 Q_uu of every step of a solve.  A CONDITION of the GPU
  tests, asserted on the CPU (test_lqr_wide_shapes_cpu.py): make_lqr_batch_fast's well-conditioned C never exchanges.
* ``launch`` / ``launch_raw``: the C ABI on NaN-filled buffers with a guard row behind the batch and a guard behind status
  (as test_lqr_pair_solve_gpu.py does): every element inside the batch comes back finite, every guard stays NaN / -1.
  The Python wrappers allocate with torch.empty and hide both an element nobody wrote and a write behind the batch.
* ``check_ratios``: the accuracy rule of test_lqr_block_gpu.py.
"""

import functools

import numpy as np

import problems
from oracle import c_oracle

NINST = 5
BUDGET = 5.0
FIELDS = ("states", "actions", "costs", "K", "k", "V", "v", "const")
ERR_UNSUPPORTED = -2

# (n, m, T); what each reaches is tabulated in DESIGN.md 3.2a
SHAPES = ((49, 16, 4),      # first d past 64: wave_for_2d with cols = 65, a second CT = 4 column group, width 66 (off the register path)
          (56, 24, 4),      # d = 80, m > 16: LDS elimination in the block kernel, ~132 KB
          (70, 4, 4),       # n > 64: ldn = 71, second trip of the row-per-lane loops
          (8, 66, 4),       # m > 64: sequential pivot search, fac filled in two trips, K = 66 / 198 product depths
          (1, 65, 4), (65, 1, 4),       # the thin edges of the same loops
          (48, 16, 53))     # the anchor: largest shape tested before, past one cost post-pass chunk of the block kernel
BOUNDARY_M = 24             # the support boundary is looked for at this m
EXTRA_PIVOTED = ((24, 24, 4),)          # shapes of test_lqr_block_gpu.py that ran the pivoted path without exchanges


# (n, m, T, (left, mid, right)): instance `mid` exchanges rows, `left` and `right` do not (asserted on the CPU)
NEIGHBOURS = (49, 16, 4, (0, 1, 4))


def pivoted(n, m):
    """The block kernel eliminates in LDS with row pivoting (the wave kernel always does)."""
    return m > 16 or m + 1 + n > 64


def seed_of(n, m):
    return SEEDS.get((n, m), 97 * n + m)


# seeds at which at least three of the five instances exchange rows (chosen on the CPU, see test_lqr_wide_shapes_cpu.py);
# shapes that are not listed meet it with the default 97 n + m
SEEDS = {(70, 4): 30,       # 97 n + m: no exchange on any instance (m = 4 under a 70-term F_u' V F_u is diagonally heavy)
         (63, 24): 1}       # 97 n + m: exchanges on two instances of five


def make_problem(n, m, B=NINST, seed=None):
    F, f, C, c, x0 = problems.make_lqr_batch_spd(B, n, m, seed=seed_of(n, m) if seed is None else seed)
    F *= 1.5 / np.sqrt(n)             # spectral radius ~1.5: unstable open loop, well inside fp32 for the Riccati sweep
    return F, f, C, c, x0


@functools.lru_cache(maxsize=None)
def case(n, m, T):
    """(problem, ref64, ref32): five instances and the two oracle solves, made once per shape and horizon, read-only."""
    problem = make_problem(n, m)
    ref64 = c_oracle.lqr_solve(*problem, T, dtype=np.float64, want_policy=True, want_value=True)
    ref32 = c_oracle.lqr_solve(*problem, T, dtype=np.float32, want_policy=True, want_value=True)
    for a in problem:
        a.setflags(write=False)
    for r in (ref64, ref32):
        for key in FIELDS:
            r[key].setflags(write=False)
    return problem, ref64, ref32


def exchanges(Q_uu):
    """Row exchanges of a Gauss-Jordan elimination of ``Q_uu`` with partial pivoting: at column p the pivot is the FIRST row
    of maximal |entry| among rows p .. m-1 (wave_gauss_jordan<true>, block_gauss_jordan<true>)."""
    A = np.array(Q_uu, dtype=np.float64)
    m = A.shape[0]
    count = 0
    for p in range(m):
        piv = p + int(np.argmax(np.abs(A[p:, p])))             # argmax returns the first maximum
        if piv != p:
            A[[p, piv]] = A[[piv, p]]
            count += 1
        A[p] /= A[p, p]
        rows = np.arange(m) != p
        A[rows] -= np.outer(A[rows, p], A[p])
    return count


def quu_sequence(F, C, V64):
    """The fp64 Q_uu of every step of one instance's solve, t = T-1 .. 0: C_uu + F_u' V_{t+1} F_u with V_T = C_xx and
    V_{t+1} from the fp64 oracle (``V64[T, n, n]``)."""
    n = F.shape[0]
    T = V64.shape[0]
    Fu = np.asarray(F, dtype=np.float64)[:, n:]
    Cd = np.asarray(C, dtype=np.float64)
    return [Cd[n:, n:] + Fu.T @ (Cd[:n, :n] if t == T - 1 else V64[t + 1]) @ Fu for t in range(T - 1, -1, -1)]


def exchange_counts(problem, V64):
    """Per instance, the exchanges summed over the steps of the solve."""
    F, _, C, _, _ = problem
    return [sum(exchanges(Q) for Q in quu_sequence(F[b], C[b], V64[b])) for b in range(F.shape[0])]


def make_permuted(n, m, B, seed):
    """Instances that cannot be solved without exchanging rows, for the general (non-symmetric C) entry points: F_u = 0 and
    C_uu = P D with P the cyclic permutation (row i holds D_i in column i + 1 mod m) -- a zero diagonal, non-symmetric;
    C_xx positive definite, C_ux and C_xu independent draws.  Then Q_uu = C_uu at every step and
    K_t = -(C_ux / D)[perm], perm[j] = j - 1 mod m: a row permutation and a scaling.
    Returns (F, f, C, c, x0, D[B, m], perm[m]) in fp64."""
    rng = np.random.default_rng(seed)
    d = n + m
    F = rng.normal(size=(B, n, d)) / np.sqrt(n)
    F[:, :, n:] = 0.0
    f = rng.normal(size=(B, n))
    c = rng.normal(size=(B, d))
    x0 = rng.normal(size=(B, n))
    A = rng.normal(size=(B, n, n))
    C = np.zeros((B, d, d))
    C[:, :n, :n] = A @ np.swapaxes(A, 1, 2) / n + np.eye(n)
    C[:, n:, :n] = 0.3 * rng.normal(size=(B, m, n))
    C[:, :n, n:] = 0.3 * rng.normal(size=(B, n, m))
    D = rng.uniform(0.5, 2.0, size=(B, m))
    rows = np.arange(m)
    C[:, n + rows, n + (rows + 1) % m] = D
    return F, f, C, c, x0, D, (rows - 1) % m


def boundary_n(lib, m=BOUNDARY_M, T=4):
    """The largest n that ``tfmpc_lqr_kernel_name`` does not call unsupported at this m, scanning down from 128."""
    for n in range(128, 0, -1):
        if lib.tfmpc_lqr_kernel_name(n, m, T) != b"unsupported":
            return n
    raise AssertionError(f"no supported n at m = {m}")


# ---- launches through the C ABI --------------------------------------------------------------------------------------

def row_shapes(n, m, T):
    """rows per instance and row width of every output, flattened to [B * rows (+ 1 guard), width]"""
    return dict(states=(T + 1, n), actions=(T, m), costs=(T + 1, 1), K=(T, m * n), k=(T, m), V=(T, n * n), v=(T, n),
                const=(T, 1))


def nan_buffers(B, n, m, T, device):
    import torch
    flat = {key: torch.full((B * r + 1, w), float("nan"), device=device) for key, (r, w) in row_shapes(n, m, T).items()}
    status = torch.full((B + 1,), -1, dtype=torch.int32, device=device)
    return flat, status


def launch_raw(lqr, x0d, B, T, flat, status, mode, general=False):
    """One entry point (``mode``: "solve", "backward", "forward") of an ``LQR``'s operands into the given buffers; returns
    the C ABI's return code.  No synchronisation."""
    from tfmpc import _hip
    lib = _hip.require_gpu()
    n, m = lqr.state_size, lqr.action_size
    sfx = "_general_f32" if general else "_f32"
    p = lambda key: _hip.ptr(flat[key])                        # noqa: E731
    if mode == "solve":
        return getattr(lib, "tfmpc_lqr_solve" + sfx)(B, n, m, T, *lqr._ptr_args(), _hip.ptr(x0d), p("states"), p("actions"),
                                                      p("costs"), p("K"), p("k"), p("V"), p("v"), p("const"),
                                                      _hip.ptr(status), None, 0, _hip.stream())
    if mode == "backward":
        return getattr(lib, "tfmpc_lqr_backward" + sfx)(B, n, m, T, *lqr._ptr_args(), p("K"), p("k"), p("V"), p("v"),
                                                         p("const"), _hip.ptr(status), _hip.stream())
    assert mode == "forward"
    return getattr(lib, "tfmpc_lqr_forward" + sfx)(B, n, m, T, *lqr._ptr_args(), p("K"), T * m * n, p("k"), T * m,
                                                    _hip.ptr(x0d), p("states"), p("actions"), p("costs"), _hip.stream())


def launch(problem, idx, T, split=False, general=False, shared=False):
    """Instances ``idx`` of ``problem`` (in that order) in one fused solve with policy and value outputs -- or, ``split``,
    one backward and one forward launch.  ``shared``: the model of instance idx[0] without a batch axis (batch stride 0)
    with the initial states of ``idx``.  Returns ({key: [B, rows, width]}, status[B]); asserts the return codes, that
    every element inside the batch is finite unless the instance is flagged, and that the guards are untouched."""
    import torch
    from tfmpc import _hip
    from tfmpc.solvers.lqr import LQR
    idx = list(idx)
    B = len(idx)
    F, f, C, c, x0 = (a[idx] for a in problem)
    n, m = F.shape[1], F.shape[2] - F.shape[1]
    lqr = LQR(F[0], f[0], C[0], c[0], symmetric=not general) if shared else LQR(F, f, C, c, symmetric=not general)
    x0d = lqr._prep_x0(x0)
    flat, status = nan_buffers(B, n, m, T, x0d.device)
    for mode in (("backward", "forward") if split else ("solve",)):
        rc = launch_raw(lqr, x0d, B, T, flat, status, mode, general)
        assert rc == 0, (n, m, T, mode, "return code", rc)
    torch.cuda.synchronize()
    what = (n, m, T, idx, "split" if split else "fused")
    out = {}
    for key, (r, w) in row_shapes(n, m, T).items():
        assert torch.isnan(flat[key][B * r:]).all(), (what, key, "guard row behind the batch")
        out[key] = flat[key][:B * r].reshape(B, r, w)
    assert int(status[B]) == -1, (what, "guard behind the status")
    st = status[:B]
    ok = (st == 0)
    assert int((st < 0).sum()) == 0, (what, "a status nobody wrote", st.tolist())
    for key in out:
        assert torch.isfinite(out[key][ok]).all(), (what, key, "an element inside the batch is not finite")
    return out, st


def ratio_stats(out, idx, ref64, ref32, fields=FIELDS):
    """{key: (median, 0.9 quantile, max)} of |gpu - fp64| / max(|fp32 oracle - fp64|, 1e-6 of the tensor's scale) per
    instance -- the rule of test_lqr_block_gpu.py."""
    stats = {}
    for key in fields:
        got = out[key].detach().cpu().numpy().astype(np.float64)
        ratios = []
        for pos, b in enumerate(idx):
            want = ref64[key][b].reshape(got[pos].shape)
            scale = np.abs(want).max()
            e32 = max(np.abs(ref32[key][b].astype(np.float64).reshape(want.shape) - want).max(), 1e-6 * scale)
            ratios.append(np.abs(got[pos] - want).max() / e32)
        stats[key] = (float(np.median(ratios)), float(np.quantile(ratios, 0.9)), float(max(ratios)))
    return stats


def check_ratios(out, idx, ref64, ref32, what, fields=FIELDS, loose=None):
    """Prints the three statistics per tensor, then asserts median <= 2, 0.9 quantile <= BUDGET, max <= 5 BUDGET.
    ``loose``: {key: factor} for a named tensor of a named shape, with the cause written where it is passed."""
    stats = ratio_stats(out, idx, ref64, ref32, fields)
    for key, (med, q9, top) in stats.items():
        print(f"{what} {key}: median {med:.2f} q0.9 {q9:.2f} max {top:.2f}")
    for key, (med, q9, top) in stats.items():
        k = (loose or {}).get(key, 1.0)
        assert np.isfinite(top), (what, key)
        assert med <= 2.0 * k and q9 <= BUDGET * k and top <= 5 * BUDGET * k, (what, key, med, q9, top)
    return stats


def same_bits(got, pos, want, wpos, what, fields=FIELDS):
    import torch
    (out, status), (wout, wstatus) = got, want
    for key in fields:
        assert torch.equal(out[key][pos], wout[key][wpos]), (what, key)
    assert int(status[pos]) == int(wstatus[wpos]), (what, "status")
