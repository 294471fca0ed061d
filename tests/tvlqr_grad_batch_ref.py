"""TEST INFRASTRUCTURE ONLY -- fp64 oracles of the BATCH-SUMMED gradients of the time-varying LQR (operands without a
batch axis: ``vjp_reduce_*`` of tf-mpc_amd/csrc/tvlqr_vjp_common.h and ``box_reduce_*`` of tvlqr_vjp.hip) at batches of more than one
reduction chunk, built on tests/tvlqr_grad_ref.py.  Shared by tests/test_tvlqr_grad_batch_cpu.py, which shows that the
references are inside every budget and bound, and tests/test_tvlqr_grad_batch_gpu.py, which holds the kernels to them.

``shared_oracle``: the fp64 sums and their budget, by the rule of ``test_tvlqr_grad_gpu._oracles`` (imported, not
restated).  ``term_magnitudes``: elementwise, the sum over the batch of the absolute products each gradient adds up --
what an fp32 summation error is relative to.  ``sum_sequential`` / ``sum_kernel_order``: fp32 sums of fp32 terms,
sequentially and in the order of the matrix-core kernel's df / dc lane sums.  ``CASES``: the (n, m, T, B, sharing)
matrix of the GPU file.
"""

import functools

import numpy as np
import torch

import lqr_box_grad_ref as bref
import tvlqr_grad_ref as gref
import tvlqr_ref
from test_tvlqr_grad_gpu import MODEL, _case, _oracles, _reduce

CHUNK = 256                       # kChunk of tvlqr_vjp_common.h: instances per stage-1 partial sum
U32 = 2.0 ** -24                  # fp32 unit roundoff

# how the operands are shared: the keywords of test_tvlqr_grad_gpu._case
SHARING = dict(batch=dict(shared=MODEL),                                 # one gradient per step
               # ... and a time axis of 1, so stage 2 also sums steps (f keeps its time axis: the horizon is read from it)
               both=dict(shared=MODEL, const=("F", "C", "c")),
               F=dict(shared=("F",)),                                    # wantC false, factor records stored
               Cc=dict(shared=("C", "c")),                               # wantF false, no factor store
               f1=dict(shared=("f",), const=("f",)),
               final=dict(final="shared", x0_shared=True),               # vjp_reduce_final / steps_stage2
               Ffc=dict(shared=("F", "f", "c")))                         # C per instance: one instance's C can be spoilt

EDGE_SHAPES = [(16, 8), (20, 10)]                  # one shape per reduction kernel (matrix cores; LDS tiles)
EDGE_BATCHES = [17, 256, 257, 519]
MFMA_SHAPES = [(16, 16), (12, 20), (16, 1), (8, 8), (5, 3), (5, 20)]     # n <= 16, d <= 32: d = 32, 32, 17, 16, 8, 25
GENERIC_SHAPES = [(17, 8), (16, 17)]               # the first shape past each dispatch condition
FINAL_SHAPES = [(16, 8), (12, 6), (20, 10)]
FINAL_BATCHES = [17, 257, 519]

BATCH_EDGE_CASES = [(n, m, 3, B, s) for (n, m) in EDGE_SHAPES for B in EDGE_BATCHES for s in ("batch", "both")]
NEED_CASES = [(n, m, 3, 519, s) for (n, m) in EDGE_SHAPES for s in ("F", "Cc", "f1")]
SHAPE_EDGE_CASES = [(n, m, 2, 519, "batch") for (n, m) in MFMA_SHAPES + GENERIC_SHAPES]
FINAL_CASES = [(n, m, 2, B, "final") for (n, m) in FINAL_SHAPES for B in FINAL_BATCHES]
CASES = BATCH_EDGE_CASES + NEED_CASES + SHAPE_EDGE_CASES + FINAL_CASES
CONSISTENCY_CASES = [(16, 8, 3, 519, "batch"), (16, 16, 2, 519, "batch"), (20, 10, 3, 519, "batch")]

# With m >= n one shared draw of the model decides the fp32 error of EVERY instance (Q_uu takes C's small eigenvalues), and
# with it the budget: over seeds 1 - 59 the one-instance separation of 5 x 20 runs from 2 to 560.  These draws are
# well-conditioned ones, so that the budget is tight enough to tell one lost instance from rounding on any host.
SEEDS = {(5, 20): 56, (12, 20): 12, (16, 16): 13}

BOX_SHAPES = [(16, 8), (5, 3), (20, 10)]
BOX_BATCH, BOX_T = 261, 2
STRIDED = dict(n=5, m=3, B=513, T=86)              # box_reduce_final's strided loop: chunks * T = 258 > 256


def case_id(case):
    n, m, T, B, sharing = case
    return f"{n}x{m}-T{T}-B{B}-{sharing}"


@functools.lru_cache(maxsize=None)
def problem(n, m, T, B, sharing):
    """-> (user operands, their [B, T, ...] broadcasts, upstream weights) of one case; mixed loss."""
    return _case(n, m, T, B, loss="mixed", seed=SEEDS.get((n, m), n + m + T + B), **SHARING[sharing])


def _args(full, w):
    return [full[k] for k in ("F", "f", "C", "c", "x0")] + [full.get("Cfin"), full.get("cfin")] + list(w)


def summed_names(user, full):
    """The gradients that are sums over the batch: operands the user passes without a batch axis."""
    return [k for k in full if np.asarray(user[k]).ndim < np.asarray(full[k]).ndim]


def shared_oracle(user, full, w):
    """-> (fp64 gradients, budget), both in the user's operand shapes: a gradient without a batch axis is the sum over
    the batch and its budget the sum of the per-instance absolute fp32 errors (C, c: fp32 autograd; F, f, x0: the larger
    of that and the fp32 closed form)."""
    return _oracles(user, full, w)


@functools.lru_cache(maxsize=None)
def oracle(n, m, T, B, sharing):
    user, full, w = problem(n, m, T, B, sharing)
    return shared_oracle(user, full, w)


def ratio(got, ref, err):
    """The project's figure for ONE instance (a summed gradient counts as one): max |got - ref| over the budget
    max(max err, 1e-6 max(1, |ref|))."""
    scale = max(1.0, float(ref.abs().max()))
    return float((got - ref).abs().max()) / max(float(err.max()), 1e-6 * scale)


def term_magnitudes(user, full, w):
    """Elementwise, in fp64 and in the user's operand shapes: the sum over the batch (and over a time axis of 1) of the
    absolute products each gradient's terms are made of,
        M_F[i,j] = sum_b |dlam_i||z_j| + |lam_i||dz_j|          M_f = sum_b |dlam|
        M_C[i,j] = sum_b (|dz_i||z_j| + |z_i||dz_j| + |gc||z_i||z_j|) / 2          M_c = sum_b |dz| + |gc||z|
    the final cost's the same in x_T, dx_T, gc_T (added at t = T - 1 when it is the default one), M_x0 = sum_b |dlam_0|."""
    _, p = gref.closed_form(*_args(full, w), parts=True)
    p = {k: v.abs() for k, v in p.items()}
    z, dz, lam, dlam, gc, xT, dxT = (p[k] for k in ("z", "dz", "lam", "dlam", "gcost", "x_T", "dx_T"))
    T, n = z.shape[1], xT.shape[-1]
    outer = lambda a, b: a.unsqueeze(-1) * b.unsqueeze(-2)                           # noqa: E731
    M = dict(F=outer(dlam, z) + outer(lam, dz), f=dlam,
             C=0.5 * (outer(dz, z) + outer(z, dz) + gc[:, :T, None, None] * outer(z, z)),
             c=dz + gc[:, :T, None] * z, x0=p["dlam_0"])
    MCf = 0.5 * (outer(dxT, xT) + outer(xT, dxT) + gc[:, T, None, None] * outer(xT, xT))
    Mcf = dxT + gc[:, T, None] * xT
    if "Cfin" in full:
        M.update(Cfin=MCf, cfin=Mcf)
    else:
        M["C"][:, T - 1, :n, :n] += MCf
        M["c"][:, T - 1, :n] += Mcf
    B = full["x0"].shape[0]
    return {k: _reduce(v, k, user, B) for k, v in M.items()}


def per_instance(user, full, w, dtype):
    """The closed form's per-instance gradients [B, T, ...] in ``dtype``, a time axis of 1 already summed (in ``dtype``,
    in time order) -- the terms a batch reduction adds up."""
    g = gref.closed_form(*_args(full, w), dtype=dtype)
    out = {}
    for k, v in g.items():
        shape = np.asarray(user[k]).shape
        if k in MODEL and shape[-3 if k in ("F", "C") else -2] == 1 and v.shape[1] != 1:
            acc = v[:, 0].clone()
            for t in range(1, v.shape[1]):
                acc = acc + v[:, t]
            v = acc.unsqueeze(1)
        out[k] = v
    return out


def sum_sequential(terms):
    """fp32: the instances one after the other."""
    acc = terms[0].clone()
    for b in range(1, terms.shape[0]):
        acc = acc + terms[b]
    return acc


def sum_kernel_order(terms):
    """fp32, the order in which vjp_reduce_steps_mfma16 and its stage 2 add up df and dc: per chunk of 256 instances four
    interleaved running sums (instance b0 + 4 g + q into lane group q), folded as ((s0 + s1) + s2) + s3; then the chunks
    in order.  (dF and dC accumulate on the matrix cores: each instruction adds its four instances and the groups go
    into one accumulator in order -- closer to ``sum_sequential``.  Either way a second fp32 order under the B u bound.)"""
    total = None
    for b0 in range(0, terms.shape[0], CHUNK):
        chunk = terms[b0:b0 + CHUNK]
        s = [torch.zeros_like(terms[0]) for _ in range(4)]
        for i in range(chunk.shape[0]):
            s[i % 4] = s[i % 4] + chunk[i]
        part = ((s[0] + s[1]) + s[2]) + s[3]
        total = part if total is None else total + part
    return total


# ---- the control-limited cases ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def box_problem(n, m):
    """``bref.tv_case`` at the batch of the box tests (explicit final cost, as the T = 2 cases of
    tests/test_lqr_box_grad_gpu.py): (operands, its own fp64 optimum)."""
    return bref.tv_case(n, m, BOX_T, BOX_BATCH, final=True)


@functools.lru_cache(maxsize=None)
def box_shared(n, m, timed):
    """Instance 0's model and bounds shared by the batch, x0 per instance, and the fp64 optimum of THAT problem.  The
    bounds are one pair per step (``timed``: passed as [T, m]) or step 0's pair at every step (passed as [m]).
    -> (operands broadcast to [B, ...], solution of ``bref.solve_box_batch``)."""
    ops, _ = box_problem(n, m)
    B, T = BOX_BATCH, BOX_T
    sh = {k: (None if v is None else np.repeat(v[:1], B, axis=0)) for k, v in ops.items() if k != "x0"}
    sh["x0"] = ops["x0"]
    if not timed:
        sh["low"], sh["high"] = sh["low"][:, :1].repeat(T, axis=1), sh["high"][:, :1].repeat(T, axis=1)
    sol = bref.solve_box_batch(sh["F"], sh["f"], sh["C"], sh["c"], sh["x0"], sh["low"], sh["high"], sh["Cfin"], sh["cfin"])
    return sh, sol


@functools.lru_cache(maxsize=None)
def all_held_rollout():
    """One time-varying model and one pair of bounds [m] shared by the batch, every control held at every step (low at
    odd steps, high at even ones): the trajectory is the rollout of the bounds, no QP solve.
    -> (operands broadcast to [B, ...] in fp64, states rounded to fp32, actions, at_low, max |x| before rounding)."""
    n, m, B, T = (STRIDED[k] for k in ("n", "m", "B", "T"))
    F, f, C, c = (np.repeat(a.astype(np.float64), B, axis=0) for a in tvlqr_ref.make_models(n, m, T, 1, seed=1))
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    lo, hi = np.full((B, T, m), -0.25), np.full((B, T, m), 0.25)
    al = np.ones((B, T, m), bool)
    al[:, ::2] = False
    us = np.where(al, lo, hi)
    xs = np.empty((B, T + 1, n))
    xs[:, 0] = x0
    for s in range(T):
        z = np.concatenate([xs[:, s], us[:, s]], -1)
        xs[:, s + 1] = np.einsum("bij,bj->bi", F[:, s], z) + f[:, s]
    exact = xs
    xs = xs.astype(np.float32).astype(np.float64)
    return dict(F=F, f=f, C=C, c=c, x0=x0, low=lo, high=hi, Cfin=None, cfin=None), xs, us, al, float(np.abs(exact).max())
