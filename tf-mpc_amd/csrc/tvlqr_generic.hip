// tvlqr_generic.hip -- shape-generic TIME-VARYING LQR (tfmpc_tvlqr_*_f32) for every shape the 16 x 8 matrix-core
// kernel does not serve (n > 16 or m > 8), up to one wave's LDS: one wavefront per instance, fp32.
//
// Per step t of the backward sweep the wave copies F_t, f_t, C_t, c_t into its LDS slice and runs the symmetric
// recursion of the fast kernels: W = F_t^T V, Q = C_t + W F_t, q = c_t + W f_t + F_t^T v on the f32
// matrix cores (wave_ops.h), Q_uu eliminated WITHOUT pivoting (a non-positive pivot <=> Q_uu not positive definite:
// TFMPC_ST_NOT_PD), V' = Q_xx + Q_xu K, v' = q_x + Q_xu k, V' symmetrised.  The rollout copies F_t, f_t, C_t, c_t, K_t,
// k_t per step.  The fallback, not a performance target: nothing is prefetched.
#include <hip/hip_runtime.h>

#include "tvlqr_kernels.h"
#include "lqr_kernels.h"
#include "wave_ops.h"

namespace tfmpc {

namespace {

struct TvSmem {
    int ldd, ldn, lda, width;
    float *F, *f, *C, *c, *V, *v, *W, *Q, *q, *aug, *fac, *prow, *K, *k, *Vn, *vn, *z, *xn;
};

__host__ __device__ inline size_t tv_smem_floats(int n, int m)
{
    const int d = n + m;
    const int ldd = odd_ld(d), ldn = odd_ld(n), width = m + 1 + n, lda = odd_ld(width);
    size_t s = 0;
    s += (size_t)n * ldd + n;          // F, f
    s += (size_t)d * ldd + d;          // C, c
    s += (size_t)n * ldn + n;          // V, v
    s += (size_t)d * ldn;              // W = F^T V
    s += (size_t)d * ldd + d;          // Q, q
    s += (size_t)m * lda + m + width;  // aug, fac, prow
    s += (size_t)m * ldn + m;          // K, k
    s += (size_t)n * ldn + n;          // Vn, vn
    s += (size_t)d + n;                // z, xn
    return s;
}

__device__ inline TvSmem tv_carve(float *base, int n, int m)
{
    TvSmem s;
    const int d = n + m;
    s.ldd = odd_ld(d);
    s.ldn = odd_ld(n);
    s.width = m + 1 + n;
    s.lda = odd_ld(s.width);
    float *p = base;
    s.F = p; p += n * s.ldd;
    s.f = p; p += n;
    s.C = p; p += d * s.ldd;
    s.c = p; p += d;
    s.V = p; p += n * s.ldn;
    s.v = p; p += n;
    s.W = p; p += d * s.ldn;
    s.Q = p; p += d * s.ldd;
    s.q = p; p += d;
    s.aug = p; p += m * s.lda;
    s.fac = p; p += m;
    s.prow = p; p += s.width;
    s.K = p; p += m * s.ldn;
    s.k = p; p += m;
    s.Vn = p; p += n * s.ldn;
    s.vn = p; p += n;
    s.z = p; p += d;
    s.xn = p; p += n;
    return s;
}

// MASKED: held controls (bit i of a.mask[b][t]) are taken out of the step's model after the LDS copy.
template <bool BACKWARD, bool FORWARD, bool MASKED>
__device__ __forceinline__ void tvlqr_generic_body(const TvLqrArgs &a, float *smem)
{
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m, T = a.T;
    TvSmem s = tv_carve(smem, n, m);
    const int ldd = s.ldd, ldn = s.ldn, lda = s.lda;
    auto load_model = [&](int t) {
        load_matrix(s.F, ldd, tv_at(a.F, a.sF_b, a.sF_t, b, t), n, d);
        load_matrix(s.C, ldd, tv_at(a.C, a.sC_b, a.sC_t, b, t), d, d);
        const float *fg = tv_at(a.f, a.sf_b, a.sf_t, b, t), *cg = tv_at(a.c, a.sc_b, a.sc_t, b, t);
        for (int i = lane; i < n; i += kWave) s.f[i] = fg[i];
        for (int i = lane; i < d; i += kWave) s.c[i] = cg[i];
    };
    // the final cost's (C_fin, c_fin, leading dimension): explicit, or C_{T-1}[:n,:n], c_{T-1}[:n]
    const float *Cf = a.Cfin ? a.Cfin + (size_t)b * a.sCfin_b : tv_at(a.C, a.sC_b, a.sC_t, b, T - 1);
    const float *cf = a.Cfin ? a.cfin + (size_t)b * a.scfin_b : tv_at(a.c, a.sc_b, a.sc_t, b, T - 1);
    const int ldf = a.Cfin ? n : d;

    int status = 0;
    float *Kg = a.K + (size_t)b * a.sK;
    float *kg = a.k + (size_t)b * a.sk;

    if (BACKWARD) {
        wave_for_2d(n, n, [&](int i, int j, int) { s.V[i * ldn + j] = Cf[i * ldf + j]; });
        for (int i = lane; i < n; i += kWave) s.v[i] = cf[i];
        float cst = 0.0f;
        wsync();

        for (int t = T - 1; t >= 0; --t) {
            load_model(t);
            wsync();
            if (MASKED) {
                const uint32_t w = a.mask[(size_t)b * T + t];
                auto held = [&](int zi) { return zi >= n && (w >> (zi - n) & 1u); };
                wave_for_2d(n, m, [&](int r, int j, int) { if (w >> j & 1u) s.F[r * ldd + n + j] = 0.0f; });
                wave_for_2d(d, d, [&](int r, int j, int) { if (held(r) || held(j)) s.C[r * ldd + j] = (r == j) ? 1.0f : 0.0f; });
                for (int r = lane; r < m; r += kWave) if (w >> r & 1u) s.c[n + r] = 0.0f;
                wsync();
            }
            // W = F_t^T V  [d][n]
            wave_matmul_mfma(d, n, n,
                        [&](int r, int k) { return s.F[k * ldd + r]; },
                        [&](int k, int j) { return s.V[k * ldn + j]; },
                        [](int, int) { return 0.0f; },
                        [&](int r, int j, float x) { s.W[r * ldn + j] = x; });
            wsync();
            // Q = C_t + W F_t ; q = c_t + W f_t + F_t^T v
            wave_matmul_mfma(d, d, n,
                        [&](int r, int k) { return s.W[r * ldn + k]; },
                        [&](int k, int j) { return s.F[k * ldd + j]; },
                        [&](int r, int j) { return s.C[r * ldd + j]; },
                        [&](int r, int j, float x) { s.Q[r * ldd + j] = x; });
            for (int r = lane; r < d; r += kWave) {
                float s1 = 0.0f, s2 = 0.0f;
                for (int k = 0; k < n; ++k) {
                    s1 = fmaf(s.W[r * ldn + k], s.f[k], s1);
                    s2 = fmaf(s.F[k * ldd + r], s.v[k], s2);
                }
                s.q[r] = s.c[r] + s1 + s2;
            }
            wsync();
            // [Q_uu | q_u | Q_ux] -> Gauss-Jordan without pivoting -> [I | Q_uu^-1 q_u | Q_uu^-1 Q_ux]
            wave_for_2d(m, s.width, [&](int r, int j, int) {
                float x;
                if (j < m) x = s.Q[(n + r) * ldd + n + j];
                else if (j == m) x = s.q[n + r];
                else x = s.Q[(n + r) * ldd + (j - m - 1)];
                s.aug[r * lda + j] = x;
            });
            wsync();
            if (wave_gauss_jordan<false>(s.aug, lda, m, s.width, s.fac, s.prow)) status |= TFMPC_ST_NOT_PD;
            wave_for_2d(m, n, [&](int r, int j, int idx) {
                const float x = -s.aug[r * lda + m + 1 + j];
                s.K[r * ldn + j] = x;
                Kg[(size_t)t * m * n + idx] = x;
            });
            for (int r = lane; r < m; r += kWave) {
                const float x = -s.aug[r * lda + m];
                s.k[r] = x;
                kg[(size_t)t * m + r] = x;
            }
            wsync();
            // V' = Q_xx + Q_xu K ; v' = q_x + Q_xu k  (Schur form; equal to lqr.py:97-105 in exact arithmetic)
            wave_matmul_mfma(n, n, m,
                        [&](int i, int k) { return s.Q[i * ldd + n + k]; },
                        [&](int k, int j) { return s.K[k * ldn + j]; },
                        [&](int i, int j) { return s.Q[i * ldd + j]; },
                        [&](int i, int j, float x) { s.Vn[i * ldn + j] = x; });
            for (int i = lane; i < n; i += kWave) {
                float s1 = 0.0f;
                for (int k = 0; k < m; ++k) s1 = fmaf(s.Q[i * ldd + n + k], s.k[k], s1);
                s.vn[i] = s.q[i] + s1;
            }
            // const += 1/2 k^T Q_uu k + k^T q_u + 1/2 f_t^T V f_t + f_t^T v (V, v before this step's update)
            float part = 0.0f;
            for (int r = lane; r < m; r += kWave) {
                float quk = 0.0f;
                for (int k = 0; k < m; ++k) quk = fmaf(s.Q[(n + r) * ldd + n + k], s.k[k], quk);
                part += s.k[r] * (0.5f * quk + s.q[n + r]);
            }
            for (int i = lane; i < n; i += kWave) {
                float vf = 0.0f;
                for (int k = 0; k < n; ++k) vf = fmaf(s.V[i * ldn + k], s.f[k], vf);
                part += s.f[i] * (0.5f * vf + s.v[i]);
            }
            cst += wave_sum(part);
            wsync();
            // V <- (V' + V'^T) / 2: the elimination above reads a symmetric Q_uu only while V stays symmetric
            wave_for_2d(n, n, [&](int i, int j, int idx) {
                const float x = 0.5f * (s.Vn[i * ldn + j] + s.Vn[j * ldn + i]);
                s.V[i * ldn + j] = x;
                if (a.V) a.V[((size_t)b * T + t) * n * n + idx] = x;
            });
            for (int i = lane; i < n; i += kWave) {
                const float x = s.vn[i];
                s.v[i] = x;
                if (a.v) a.v[((size_t)b * T + t) * n + i] = x;
            }
            if (a.cst && lane == 0) a.cst[(size_t)b * T + t] = cst;
            wsync();
        }
        if (!(cst == cst)) status |= TFMPC_ST_NAN;
    }

    if (FORWARD) {
        float *xs = a.states + (size_t)b * (T + 1) * n;
        float *us = a.actions + (size_t)b * T * m;
        float *cs = a.costs + (size_t)b * (T + 1);
        __syncthreads();                                 // gains written above are visible
        for (int i = lane; i < n; i += kWave) {
            const float x = a.x0[(size_t)b * n + i];
            s.z[i] = x;
            xs[i] = x;
        }
        for (int t = 0; t < T; ++t) {
            load_model(t);
            load_matrix(s.K, ldn, Kg + (size_t)t * m * n, m, n);
            for (int r = lane; r < m; r += kWave) s.k[r] = kg[(size_t)t * m + r];
            wsync();
            for (int r = lane; r < m; r += kWave) {        // u = K_t x + k_t
                float u = s.k[r];
                for (int j = 0; j < n; ++j) u = fmaf(s.K[r * ldn + j], s.z[j], u);
                s.z[n + r] = u;
                us[(size_t)t * m + r] = u;
            }
            wsync();
            float part = 0.0f;                             // 1/2 z^T C_t z + c_t^T z
            for (int r = lane; r < d; r += kWave) {
                float cz = 0.0f;
                for (int j = 0; j < d; ++j) cz = fmaf(s.C[r * ldd + j], s.z[j], cz);
                part += s.z[r] * (0.5f * cz + s.c[r]);
            }
            for (int i = lane; i < n; i += kWave) {        // x' = F_t z + f_t
                float x = s.f[i];
                for (int j = 0; j < d; ++j) x = fmaf(s.F[i * ldd + j], s.z[j], x);
                s.xn[i] = x;
            }
            const float cost = wave_sum(part);
            if (lane == 0) cs[t] = cost;
            wsync();
            for (int i = lane; i < n; i += kWave) {
                const float x = s.xn[i];
                s.z[i] = x;
                xs[(size_t)(t + 1) * n + i] = x;
            }
            wsync();
        }
        float part = 0.0f;                                 // 1/2 x^T C_fin x + c_fin^T x
        for (int r = lane; r < n; r += kWave) {
            float cz = 0.0f;
            for (int j = 0; j < n; ++j) cz = fmaf(Cf[r * ldf + j], s.z[j], cz);
            part += s.z[r] * (0.5f * cz + cf[r]);
        }
        const float last_cost = wave_sum(part);
        if (lane == 0) cs[T] = last_cost;
        if (!(last_cost == last_cost)) status |= TFMPC_ST_NAN;
    }

    if (a.status && lane == 0) a.status[b] = status;
}

template <bool BACKWARD, bool FORWARD>
__global__ __launch_bounds__(kWave) void tvlqr_generic_kernel(TvLqrArgs a)
{
    extern __shared__ float smem[];
    tvlqr_generic_body<BACKWARD, FORWARD, false>(a, smem);
}

// The fused solve on a masked model (tvlqr_solve_masked_f32).
__global__ __launch_bounds__(kWave) void tvlqr_generic_masked_sweep(TvLqrArgs a)
{
    extern __shared__ float smem[];
    tvlqr_generic_body<true, true, true>(a, smem);
}

template <bool BW, bool FW>
int launch(const TvLqrArgs &a, hipStream_t stream)
{
    const size_t smem = tvlqr_generic_smem_bytes(a.n, a.m);
    if (smem > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
    auto kern = tvlqr_generic_kernel<BW, FW>;
    if (smem > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)smem) != hipSuccess)
            return TFMPC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(a.B), dim3(kWave), smem, stream, a);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

}  // namespace

size_t tvlqr_generic_smem_bytes(int n, int m) { return tv_smem_floats(n, m) * sizeof(float); }

int tvlqr_generic_launch(const TvLqrArgs &a, bool backward, bool forward, hipStream_t stream)
{
    if (a.mask) {
        if (!(backward && forward) || a.V || a.v || a.cst) return TFMPC_ERR_ARG;
        const size_t smem = tvlqr_generic_smem_bytes(a.n, a.m);
        if (smem > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
        if (smem > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(tvlqr_generic_masked_sweep),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
            return TFMPC_ERR_LAUNCH;
        hipLaunchKernelGGL(tvlqr_generic_masked_sweep, dim3(a.B), dim3(kWave), smem, stream, a);
        return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
    }
    if (backward && forward) return launch<true, true>(a, stream);
    if (backward) return launch<true, false>(a, stream);
    return launch<false, true>(a, stream);
}

}  // namespace tfmpc
