"""TEST INFRASTRUCTURE ONLY -- numpy float64 emulation of the shared batch sum of tf-mpc_amd/csrc/batch_sum.h (DESIGN.md
3.13) as the double gradients instantiate it: the order of tests/batch_sum_ref.py (which casts to float32 and serves the
fp32 kernels), every accumulator a double.  tests/test_lqr_steady_state_grad_f64_cpu.py checks the emulation itself,
tests/test_lqr_steady_state_grad_f64_gpu.py holds the kernels to it bit for bit.

Records are ``rec[B, nE]`` (any trailing shape is flattened).  Every sum starts from +0.0 and adds one float64 at a time.
"""

import numpy as np

import batch_sum_ref

STEADY_STATE_CHUNK = batch_sum_ref.STEADY_STATE_CHUNK     # tfmpc_lqr_steady_state_vjp_f64: stage 1 over 64 instances, tree stage 2
THREADS = batch_sum_ref.THREADS


def stage1(rec, chunk):
    """partial[k, e]: over the instances b0 = k chunk <= b < min(B, b0 + chunk) four interleaved running sums (instance
    b0 + 4 i + q into s[q]; the instances left after the last full group of four into s[0], s[1], s[2]), then
    (s[0] + s[1]) + (s[2] + s[3])."""
    rec = np.asarray(rec, dtype=np.float64)
    rec = rec.reshape(rec.shape[0], -1)
    B, nE = rec.shape
    partial = np.empty((-(-B // chunk), nE), np.float64)
    for k in range(partial.shape[0]):
        b0, b1 = k * chunk, min(B, (k + 1) * chunk)
        s = np.zeros((4, nE), np.float64)
        bb = b0
        while bb + 4 <= b1:
            for q in range(4):
                s[q] += rec[bb + q]
            bb += 4
        for q in range(b1 - bb):
            s[q] += rec[bb + q]
        partial[k] = (s[0] + s[1]) + (s[2] + s[3])
    return partial


def stage2_tree(partial):
    """out[e]: thread t of 256 adds chunks t, t + 256, t + 512, ... in that order; then the halving tree
    t[i] += t[i + w] for i < w, w = 128, 64, ..., 1."""
    t = np.zeros((THREADS, partial.shape[1]), np.float64)
    for k, row in enumerate(partial):
        t[k % THREADS] += row
    w = THREADS // 2
    while w:
        t[:w] += t[w:2 * w]
        w //= 2
    return t[0].copy()


def steady_state_sum(per_instance):
    """The bits tfmpc_lqr_steady_state_vjp_f64 writes for a summed output, from its per-instance gradients [B, ...]."""
    per_instance = np.asarray(per_instance, dtype=np.float64)
    return stage2_tree(stage1(per_instance, STEADY_STATE_CHUNK)).reshape(per_instance.shape[1:])
