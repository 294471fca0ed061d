"""TEST INFRASTRUCTURE ONLY -- numpy float32 emulation of the shared batch sum of tf-mpc_amd/csrc/batch_sum.h (DESIGN.md
3.13): the exact order in which a gradient whose batch stride is 0 is added up from its per-instance records, and the
workspace the sum needs.  tests/test_batch_sum_cpu.py checks the emulation itself, tests/test_batch_sum_gpu.py holds the
kernels to it bit for bit.

Records are ``rec[B, nE]`` (any trailing shape is flattened).  Every sum starts from +0.0 and adds one float32 at a time.
"""

import numpy as np

STEADY_STATE_CHUNK = 64           # tfmpc_lqr_steady_state_vjp_f32: stage 1 over 64 instances, tree stage 2
RICCATI_CHUNK = 256               # tfmpc_tvlqr_backward_vjp_f32: stage 1 over 256 instances, in-order stage 2
THREADS = 256                     # kSumThreads: the width of the tree stage 2


def stage1(rec, chunk):
    """partial[k, e]: over the instances b0 = k chunk <= b < min(B, b0 + chunk) four interleaved running sums (instance
    b0 + 4 i + q into s[q]; the instances left after the last full group of four into s[0], s[1], s[2]), then
    (s[0] + s[1]) + (s[2] + s[3])."""
    rec = np.asarray(rec, dtype=np.float32)
    rec = rec.reshape(rec.shape[0], -1)
    B, nE = rec.shape
    partial = np.empty((-(-B // chunk), nE), np.float32)
    for k in range(partial.shape[0]):
        b0, b1 = k * chunk, min(B, (k + 1) * chunk)
        s = np.zeros((4, nE), np.float32)
        bb = b0
        while bb + 4 <= b1:
            for q in range(4):
                s[q] += rec[bb + q]
            bb += 4
        for q in range(b1 - bb):
            s[q] += rec[bb + q]
        partial[k] = (s[0] + s[1]) + (s[2] + s[3])
    return partial


def stage2_in_order(partial):
    """out[e] = the chunks' partial sums one after the other, chunk 0 first."""
    out = np.zeros(partial.shape[1], np.float32)
    for row in partial:
        out += row
    return out


def stage2_tree(partial):
    """out[e]: thread t of 256 adds chunks t, t + 256, t + 512, ... in that order; then the halving tree
    t[i] += t[i + w] for i < w, w = 128, 64, ..., 1."""
    t = np.zeros((THREADS, partial.shape[1]), np.float32)
    for k, row in enumerate(partial):
        t[k % THREADS] += row
    w = THREADS // 2
    while w:
        t[:w] += t[w:2 * w]
        w //= 2
    return t[0].copy()


def steady_state_sum(per_instance):
    """The bits tfmpc_lqr_steady_state_vjp_f32 writes for a summed output, from its per-instance gradients [B, ...]."""
    per_instance = np.asarray(per_instance, dtype=np.float32)
    return stage2_tree(stage1(per_instance, STEADY_STATE_CHUNK)).reshape(per_instance.shape[1:])


def riccati_sum(per_instance):
    """The bits tfmpc_tvlqr_backward_vjp_f32 writes for a summed output, from its per-instance gradients [B, ...]."""
    per_instance = np.asarray(per_instance, dtype=np.float32)
    return stage2_in_order(stage1(per_instance, RICCATI_CHUNK)).reshape(per_instance.shape[1:])


def up64(x):
    return (x + 63) // 64 * 64


def workspace_floats(B, chunk, outputs):
    """``outputs``: (size, slots) of every summed output, in output order.  One record array [B][slots][size] per output,
    each rounded up to 64 floats, then the stage-1 partial sums of the widest output (every output reuses them)."""
    if not outputs:
        return 0
    chunks = -(-B // chunk)
    return sum(up64(B * slots * size) for size, slots in outputs) + up64(chunks * max(size * slots for size, slots in outputs))


def steady_state_workspace_bytes(B, n, m):
    d = n + m
    return 4 * workspace_floats(B, STEADY_STATE_CHUNK, [(n * d, 1), (n, 1), (d * d, 1), (d, 1)])


def riccati_workspace_bytes(B, n, m, T):
    d = n + m
    return 4 * workspace_floats(B, RICCATI_CHUNK, [(n * d, T), (n, T), (d * d, T), (d, T), (n * n, 1), (n, 1)])
