"""The ground under tests/test_ilqr_lq_horizon_gpu.py, checked without a GPU:

* the constants the horizons are derived from are the ones in the kernel sources (chunk 48 and rings of ilqr_lq_mfma32.hip; ring
  depths, the z row stride and the 40 KB cap of ilqr_lq_mfma.hip; ring and 48 KB cap of ilqr_lq_box_mfma.hip), and the two LDS-byte
  formulas restated in Python put the last admitted horizons at T = 187 and T = 148;
* the workload is SAFE for the reference: at every horizon of the GPU file the fp32 restatement of ilqr.py makes the fp64 one's number
  of iterations on every unbounded instance (on >= 80 % of the bounded ones), and the open-loop start rollout stays finite to T = 1000;
* the workload SEES the faults the GPU tests are for.  The defect model (tests/ilqr_lq_horizon_ref.py) injects ONE wrong step into the
  first line-search rollout under the gains of the first backward pass.  On an LQ problem that rollout IS the solution (one Newton step,
  then a pass that only confirms), so what the fault moves is what the GPU test compares with fp64.  A position counts as visible when
  the fault moves some asserted field on some instance by >= 100 x its budget: 10 x the largest ratio the GPU assertion lets through.

What is hidden (``HIDDEN`` below, asserted): a wrong GAIN index is visible at every boundary step of every horizon, mid-horizon too -- the
first pass's k_t follows the random start actions and differs from step to step (unlike the LQR solve's stationary gains).  The CARRIED
ROW of ilqr_lq_mfma32's chunks is visible only where the chunk starts in the final transient (T = 49 .. 52, 97, 99, 145: the boundary
1 - 4 steps before the end); in mid-horizon x_{t-1} and x_t are both at the closed loop's fixed point: the 9 earlier chunk starts of
the horizons 97 .. 257 (per shape) and all 20 of T = 1000 are dropped as provably hidden.  Every boundary kind of every kernel keeps a visible horizon.
"""

import os
import re

import numpy as np
import pytest

import ilqr_lq_horizon_ref as ref
from oracle import ilqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tf-mpc_amd", "csrc")
VISIBLE = 10.0 * ref.MAX_BAR
N_SENS = 4                          # instances (the first of the GPU case's batch) the sensitivity is measured on

# (kernel, n, m, form, horizons, bound): every case family of the GPU file
FAMILIES = ([("lq_mfma", 16, 8, "exact", ref.T_LQ_EXACT, None)] +
            [("lq_mfma", n, m, "generic", ref.T_LQ_GENERIC, None) for n, m in ref.SHAPES_LQ_GENERIC] +
            [("lq_box_mfma", n, m, "exact", ref.T_BOX, ref.BOUND) for n, m in ref.SHAPES_BOX] +
            [("lq_mfma32", n, m, "exact", ref.T_MFMA32, None) for n, m in ref.SHAPES_MFMA32])
IDS = [f"{k}-{n}x{m}-{form}" for k, n, m, form, _, _ in FAMILIES]

# chunk starts of ilqr_lq_mfma32 whose carried row is hidden, per shape: {T: steps}.  Measured: <= 1e-3 of the budget in mid-horizon, 15 - 80 x at T = 257, step 240 (17 steps before the end).
HIDDEN = {97: (48,), 99: (48,), 145: (48, 96), 257: (48, 96, 144, 192, 240)}


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_are_the_kernel_sources():
    src, box, big = _source("ilqr_lq_mfma.hip"), _source("ilqr_lq_box_mfma.hip"), _source("ilqr_lq_mfma32.hip")
    (tc,) = re.findall(r"^constexpr\s+int\s+kTC\s*=\s*(\d+)\s*;", big, flags=re.M)
    assert int(tc) == ref.LQ_MFMA32["chunk"] == 48
    assert re.findall(r"constexpr\s+int\s+kRing\s*=\s*(.+?);", big) == ["REUSE ? 4 : 1"]
    assert (ref.LQ_MFMA32["ring"], ref.LQ_MFMA32["ring_no_reuse"]) == (4, 1)
    # both rings of ilqr_lq_mfma.hip (the gain-reusing sweep's and the rollout's) have the one depth
    assert re.findall(r"constexpr\s+int\s+kDepth\s*=\s*(.+?);", src) == ["EXACT ? 4 : 2"] * 2
    assert (ref.LQ_MFMA["ring_exact"], ref.LQ_MFMA["ring_generic"]) == (4, 2)
    (zld,) = re.findall(r"^#define\s+TFMPC_LQ_ZLD\s+(\d+)\s*$", src, flags=re.M)
    assert int(zld) == ref.LQ_MFMA["kZld"] == 24
    assert not re.search(r"TFMPC_LQ_ZLD", _source("Makefile"))                   # the build does not override it
    assert re.search(r"ilqr_lq_mfma_lds_bytes\(T\)\s*<=\s*40 \* 1024", src) and ref.LQ_MFMA["cap"] == 40 * 1024
    assert re.findall(r"constexpr\s+int\s+kGainRing\s*=\s*(\d+)\s*;", box) == ["4"] and ref.LQ_BOX["ring"] == 4
    assert re.search(r"box_lds_bytes\(T\)\s*<=\s*48 \* 1024", box) and ref.LQ_BOX["cap"] == 48 * 1024
    (zld_box,) = re.findall(r"^constexpr\s+int\s+kZld\s*=\s*(\d+)\s*;", box, flags=re.M)
    assert int(zld_box) == ref.LQ_BOX["kZld"]
    # the two byte formulas as the sources write them, and the operand floats in front of the trajectories
    assert "(kDyn + 2 * Tp * kZld + 2 * ((Tp + 3) & ~(size_t)3) + 8) * sizeof(float)" in src
    assert "(kDyn + 3 * Tp * kZld + 3 * ((Tp + 3) & ~(size_t)3) + 8) * sizeof(float)" in box
    assert re.search(r"kVt = 512, kVtLd = 20, kDyn = kVt \+ 16 \* kVtLd;", src) and ref.LQ_MFMA["kDyn"] == 832
    assert re.search(r"kVt = 768, kVtLd = 20, kDyn = kVt \+ 16 \* kVtLd;", box) and ref.LQ_BOX["kDyn"] == 1088


def test_the_lds_caps_admit_187_and_148_steps():
    assert ref.t_max(ref.LQ_MFMA) == ref.T_SWITCH_LQ == 187 and ref.t_max(ref.LQ_BOX) == ref.T_SWITCH_BOX == 148
    assert ref.lds_bytes(ref.LQ_MFMA, 187) == 40960 and ref.lds_bytes(ref.LQ_MFMA, 188) > 40960       # exactly the cap
    assert ref.lds_bytes(ref.LQ_BOX, 148) <= 49152 < ref.lds_bytes(ref.LQ_BOX, 149)
    # the horizon lists stand where they were chosen to: on the caps, below every ring, T mod 4 = 1, around the chunks of 48
    assert {186, 187} <= set(ref.T_LQ_EXACT) and {147, 148} <= set(ref.T_BOX) and 187 in ref.T_LQ_GENERIC
    for hs, ring in ((ref.T_LQ_EXACT, 4), (ref.T_LQ_GENERIC, 2), (ref.T_BOX, 4), (ref.T_MFMA32, 4)):
        assert set(range(1, ring)) <= set(hs) and any(T > ring and T % ring == 1 for T in hs)
    c = ref.LQ_MFMA32["chunk"]
    assert {c - 1, c, c + 1, c + 2, c + 3, c + 4, 2 * c + 1, 2 * c + 3, 3 * c + 1} <= set(ref.T_MFMA32)


def test_defect_free_rollout_is_the_oracles_forward():
    for n, m, T, bound in ((16, 8, 13, None), (17, 9, 51, None), (12, 6, 9, ref.BOUND)):
        F, f, C, c, x0, u0 = ref.workload(2, n, m, 3, T, bound)
        o, x_hat, u_hat, K, k = ref.first_pass(F[1], f[1], C[1], c[1], x0[1], u0[1], bound)
        for alpha in (1.0, 0.25):
            got = ref.rollout(o, x_hat, u_hat, K, k, alpha)
            xs, us, cs, _, _ = o.forward(x_hat, u_hat, K, k, alpha)
            for name, want in zip(ref.FIELDS, (xs[..., 0], us[..., 0], cs)):
                assert np.abs(got[name] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (n, m, name)
        # a fault changes the step it is injected at and nothing before it
        bad = ref.rollout(o, x_hat, u_hat, K, k, gain_of={5: 4})
        good = ref.rollout(o, x_hat, u_hat, K, k)
        assert np.array_equal(bad["actions"][:5], good["actions"][:5]) and not np.array_equal(bad["actions"][5], good["actions"][5])


@pytest.mark.parametrize("kernel,n,m,form,horizons,bound", FAMILIES, ids=IDS)
def test_fp32_restatement_makes_the_fp64_iterations(kernel, n, m, form, horizons, bound):
    """Every horizon of the GPU file (the switch horizons 188 / 149 and T = 1000 included), the GPU file's own instances."""
    horizons = list(horizons)
    if kernel == "lq_mfma" and (n, m) == (16, 8) and form == "exact":
        horizons.append(ref.T_SWITCH_LQ + 1)
    if kernel == "lq_box_mfma" and (n, m) == (16, 8):
        horizons.append(ref.T_SWITCH_BOX + 1)
    if (kernel, n, m) == ("lq_mfma32", 32, 16):
        horizons.append(ref.T_LONG)
    for T in horizons:
        B = ref.batch_of(T, bound is not None)
        r64, r32 = ref.oracle(n, m, T, ref.seed_of(n, m), B, bound)
        same = np.array([a["iterations"] == b["iterations"] for a, b in zip(r64, r32)])
        if bound is None:
            assert same.all(), (T, [(a["iterations"], b["iterations"]) for a, b in zip(r64, r32)])
            assert all(a["iterations"] == 1 for a in r64), T               # one Newton step and the pass that confirms it
        else:
            assert same.mean() >= 0.8, (T, same.mean())
            on_bound = np.mean([np.mean(np.abs(a["actions"]) >= bound - 1e-12) for a in r64])
            print(f"{kernel} ({n}, {m}) T={T}: {on_bound:.2f} of the final actions on the bound, iterations {[a['iterations'] for a in r64]}")
            assert all(np.abs(a["actions"]).max() <= bound for a in r64)
        for a, b in zip(r64, r32):
            for name in ref.FIELDS:
                assert np.isfinite(a[name]).all() and np.isfinite(b[name]).all(), (T, name)
                if bound is None:                                       # the budget is rounding (bounded: two solves stopped by atol = 5e-3)
                    assert ref.budget(a, b, name) <= 1e-5 * max(1.0, np.abs(a[name]).max()), (T, name)


def test_share_of_final_actions_on_the_bound():
    """A third to a half, over the horizons of a shape (single short horizons scatter around it)."""
    for n, m in ref.SHAPES_BOX:
        on, total = 0, 0
        for T in ref.T_BOX:
            r64, _ = ref.oracle(n, m, T, ref.seed_of(n, m), ref.batch_of(T, True), ref.BOUND)
            on += sum(int((np.abs(a["actions"]) >= ref.BOUND - 1e-12).sum()) for a in r64)
            total += sum(a["actions"].size for a in r64)
        print(f"({n}, {m}): {on / total:.3f} of the final actions on the bound")
        assert 1 / 3 <= on / total <= 1 / 2, (n, m, on / total)


def test_the_unreachable_tolerance_is_reachable_in_fp64():
    """atol = 1e-12, max_iterations = 4 is meant to make every instance run all four passes (three gain-reusing ones in a row).  The
    fp64 restatement DOES reach 1e-12 and stops after the confirming pass (iteration 1).  The fp32 one cannot reach it by converging:
    its later passes run on rounding noise, and it stops at 1, 2 or 3 depending on whether a line search at the noise floor rejects
    every step (regularisation then grows until k_t vanishes below the tolerance).  So no fp32 program's count can be held to a
    reference in that configuration: the GPU file holds it to 1 .. 3 (never fewer passes than fp64) and holds the TRAJECTORY, which
    is the same optimum in every case, to the fp64 one by the budget rule."""
    counts = set()
    for n, m, T in ((16, 8, 13), (17, 9, 49)):
        r64, r32 = ref.oracle(n, m, T, ref.seed_of(n, m), ref.batch_of(T), None, ref.ATOL_CONFIG)
        assert all(a["iterations"] == 1 for a in r64) and all(1 <= b["iterations"] <= 3 for b in r32)
        counts |= {b["iterations"] for b in r32}
        d64, _ = ref.oracle(n, m, T, ref.seed_of(n, m), ref.batch_of(T), None)
        for a, d, b in zip(r64, d64, r32):
            assert np.abs(a["states"] - d["states"]).max() <= 1e-9 * np.abs(d["states"]).max()
            assert np.abs(b["states"] - d["states"]).max() <= 1e-5 * np.abs(d["states"]).max()
    assert 3 in counts and len(counts) > 1, counts


@pytest.mark.parametrize("n,m", ref.SHAPES_MFMA32 + ((16, 8), (12, 6)))
def test_start_rollout_stays_bounded_to_1000_steps(n, m):
    T, B = ref.T_LONG, ref.batch_of(ref.T_LONG)
    F, f, C, c, x0, u0 = ref.workload(B, n, m, ref.seed_of(n, m), T)
    for b in range(B):
        for dtype in (np.float64, np.float32):
            x, u, cs = ref._solver(F[b], f[b], C[b], c[b], None, dtype, ()).start(x0[b], T, u_init=u0[b][..., None])
            assert np.isfinite(x).all() and np.isfinite(cs).all() and np.abs(x).max() <= 1e3 and np.abs(cs).max() <= 1e6, (b, dtype)


@pytest.mark.parametrize("kernel,n,m,form,horizons,bound", FAMILIES, ids=IDS)
def test_a_wrong_step_at_every_boundary_is_seen(kernel, n, m, form, horizons, bound):
    ring = ref.ring_of(kernel, n, m, form)
    chunk = ref.LQ_MFMA32["chunk"] if kernel == "lq_mfma32" else None
    horizons = list(horizons) + ([ref.T_LONG] if (kernel, n, m) == ("lq_mfma32", 32, 16) else [])
    visible_kinds, hidden, worst = set(), {}, np.inf
    for T in horizons:
        B = ref.batch_of(T, bound is not None)
        F, f, C, c, x0, u0 = ref.workload(B, n, m, ref.seed_of(n, m), T, bound)
        r64, r32 = ref.oracle(n, m, T, ref.seed_of(n, m), B, bound)
        idx = range(min(N_SENS, B))
        first = [ref.first_pass(F[b], f[b], C[b], c[b], x0[b], u0[b], bound) for b in idx]
        healthy = [ref.rollout(*p) for p in first]
        if bound is None:           # the model's premise: the healthy first rollout is the solution, far inside the budget
            assert max(ref.defect_ratio(healthy[b], r64[b], r64[b], r32[b]) for b in idx) <= 1e-3, T
        steps = ref.boundary_steps(T, ring, chunk)
        if T == ref.T_LONG:         # the long case: its chunk starts alone (the ring's ends are every other horizon's)
            steps = {t: kind for t, kind in steps.items() if kind == "chunk-start"}
        for t, kind in steps.items():
            for name, kw in ref.defects(t, kind, T).items():
                r = max(ref.defect_ratio(healthy[b], ref.rollout(*first[b], **kw), r64[b], r32[b]) for b in idx)
                what = "carry" if name == "row one early" else "gain"
                if r >= VISIBLE:
                    visible_kinds.add((kind, what))
                    worst = min(worst, r)
                else:
                    assert what == "carry", (T, t, kind, name, r)                    # no wrong gain index is hidden anywhere
                    hidden.setdefault(T, []).append(t)
    print(f"{kernel} ({n}, {m}) {form}: smallest visible fault / budget {worst:.3g}; hidden carried rows {hidden}")
    if chunk is None:
        assert not hidden
        want = {("prologue", "gain"), ("last-prefetch", "gain")}
    else:
        expect = {**HIDDEN, **({ref.T_LONG: tuple(range(48, 1000, 48))} if ref.T_LONG in horizons else {})}
        assert {T: tuple(sorted(ts)) for T, ts in hidden.items()} == expect
        want = {("prologue", "gain"), ("last-prefetch", "gain"), ("chunk-start", "gain"), ("chunk-start", "carry")}
        # the horizons that keep the carried row visible: the boundary 1 - 4 steps before the end, after one, two and three chunks
        assert set(horizons) - set(hidden) >= {49, 50, 51, 52}
    assert visible_kinds == want, visible_kinds
