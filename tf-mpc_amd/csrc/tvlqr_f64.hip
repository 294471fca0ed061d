// tvlqr_f64.hip -- DOUBLE-PRECISION time-varying LQR (tfmpc_tvlqr_*_f64): the wave-per-instance
// twin of tvlqr_generic.hip with every value in double, and its extern "C" entry points.
//
// Per step t of the backward sweep the wave copies F_t, f_t, C_t, c_t into its LDS slice and runs the symmetric
// recursion of DESIGN.md 3.7: W = F_t^T V, Q = C_t + W F_t and V' = Q_xx + Q_xu K on v_mfma_f64_16x16x4_f64
// (wave_ops_f64.h), q = c_t + W f_t + F_t^T v, v' and const on the vector unit, Q_uu eliminated WITHOUT pivoting (a
// non-positive pivot <=> Q_uu not positive definite: TFMPC_ST_NOT_PD), V' symmetrised.  The rollout copies F_t, f_t,
// C_t, c_t, K_t, k_t per step.  n <= 32 and m <= 32; nothing is prefetched.  The split backward + forward launches and
// the fused solve run the same device function and give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lqr_kernels.h"
#include "wave_ops_f64.h"
#include "../../include/tfmpc_hip.h"

namespace tfmpc {

namespace {

constexpr int kTvF64MaxDim = 32;

// Model operand X of instance b at step t starts at X + b * sX_b + t * sX_t (elements; 0 = shared / constant).
struct TvLqrArgsF64 {
    int B, n, m, T;
    const double *F, *f, *C, *c;
    long sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t;
    const double *Cfin, *cfin;    // final cost [n][n], [n]; both NULL: C_{T-1}[:n,:n], c_{T-1}[:n]
    long sCfin_b, scfin_b;
    const double *x0;
    double *K, *k;                // [B][T][m][n], [B][T][m]
    long sK, sk;                  // batch strides of K, k (forward-only launches may share a policy: 0)
    double *V, *v, *cst;          // optional value-function outputs [B][T][n][n], [B][T][n], [B][T]
    double *states, *actions, *costs;
    int32_t *status;
};

__device__ inline const double *tv_at(const double *p, long sb, long st, int b, int t)
{
    return p + (size_t)b * sb + (size_t)t * st;
}

struct TvSmemF64 {
    int ldd, ldn, lda, width;
    double *F, *f, *C, *c, *V, *v, *W, *Q, *q, *aug, *fac, *K, *k, *vn, *z, *xn;
};

// The layout of tvlqr_generic.hip in doubles, with three of its buffers folded into others (LDS, not registers, sets the
// resident waves here): Q is written over C_t (each lane replaces the element it read as the product's
// initial value), V' over Q_xx in the same way, and the elimination's augmented system takes W's place once Q and q
// are formed.  n = 16, m = 8: 1 968 doubles = 15.4 KiB, ten waves per CU; n = m = 32: 10 848 doubles = 84.75 KiB, one.
__host__ __device__ inline size_t tv_w_doubles(int n, int m)
{
    const size_t w = (size_t)(n + m) * odd_ld(n), aug = (size_t)m * odd_ld(m + 1 + n);
    return w > aug ? w : aug;
}

__host__ __device__ inline size_t tv_smem_doubles(int n, int m)
{
    const int d = n + m;
    const int ldd = odd_ld(d), ldn = odd_ld(n);
    size_t s = 0;
    s += (size_t)n * ldd + n;          // F, f
    s += (size_t)d * ldd + d;          // C (then Q, then V' in Q_xx), c
    s += (size_t)n * ldn + n;          // V, v
    s += tv_w_doubles(n, m);           // W = F^T V, then aug
    s += (size_t)d + m;                // q, fac
    s += (size_t)m * ldn + m;          // K, k
    s += (size_t)n;                    // vn
    s += (size_t)d + n;                // z, xn
    return s;
}

__device__ inline TvSmemF64 tv_carve(double *base, int n, int m)
{
    TvSmemF64 s;
    const int d = n + m;
    s.ldd = odd_ld(d);
    s.ldn = odd_ld(n);
    s.width = m + 1 + n;
    s.lda = odd_ld(s.width);
    double *p = base;
    s.F = p; p += n * s.ldd;
    s.f = p; p += n;
    s.C = p; p += d * s.ldd;
    s.c = p; p += d;
    s.V = p; p += n * s.ldn;
    s.v = p; p += n;
    s.Q = s.C;
    s.W = p; s.aug = p; p += tv_w_doubles(n, m);
    s.q = p; p += d;
    s.fac = p; p += m;
    s.K = p; p += m * s.ldn;
    s.k = p; p += m;
    s.vn = p; p += n;
    s.z = p; p += d;
    s.xn = p; p += n;
    return s;
}

// MAXD: the compile-time bound on n and m (16 or 32), i.e. on the k-steps of every matrix product.
template <int MAXD, bool BACKWARD, bool FORWARD>
__device__ __forceinline__ void tvlqr_f64_body(const TvLqrArgsF64 &a, double *smem)
{
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m, T = a.T;
    TvSmemF64 s = tv_carve(smem, n, m);
    const int ldd = s.ldd, ldn = s.ldn, lda = s.lda;
    auto load_model = [&](int t) {
        load_matrix_f64(s.F, ldd, tv_at(a.F, a.sF_b, a.sF_t, b, t), n, d);
        load_matrix_f64(s.C, ldd, tv_at(a.C, a.sC_b, a.sC_t, b, t), d, d);
        const double *fg = tv_at(a.f, a.sf_b, a.sf_t, b, t), *cg = tv_at(a.c, a.sc_b, a.sc_t, b, t);
        for (int i = lane; i < n; i += kWave) s.f[i] = fg[i];
        for (int i = lane; i < d; i += kWave) s.c[i] = cg[i];
    };
    // the final cost's (C_fin, c_fin, leading dimension): explicit, or C_{T-1}[:n,:n], c_{T-1}[:n]
    const double *Cf = a.Cfin ? a.Cfin + (size_t)b * a.sCfin_b : tv_at(a.C, a.sC_b, a.sC_t, b, T - 1);
    const double *cf = a.Cfin ? a.cfin + (size_t)b * a.scfin_b : tv_at(a.c, a.sc_b, a.sc_t, b, T - 1);
    const int ldf = a.Cfin ? n : d;

    int status = 0;
    double *Kg = a.K + (size_t)b * a.sK;
    double *kg = a.k + (size_t)b * a.sk;

    if (BACKWARD) {
        wave_for_2d(n, n, [&](int i, int j, int) { s.V[i * ldn + j] = Cf[i * ldf + j]; });
        for (int i = lane; i < n; i += kWave) s.v[i] = cf[i];
        double cst = 0.0;
        wsync();

        for (int t = T - 1; t >= 0; --t) {
            load_model(t);
            wsync();
            // W = F_t^T V  [d][n]
            wave_matmul_f64<MAXD>(d, n, n,
                        [&](int r, int k) { return s.F[k * ldd + r]; },
                        [&](int k, int j) { return s.V[k * ldn + j]; },
                        [](int, int) { return 0.0; },
                        [&](int r, int j, double x) { s.W[r * ldn + j] = x; });
            wsync();
            // Q = C_t + W F_t, over C_t ; q = c_t + W f_t + F_t^T v
            wave_matmul_f64<MAXD>(d, d, n,
                        [&](int r, int k) { return s.W[r * ldn + k]; },
                        [&](int k, int j) { return s.F[k * ldd + j]; },
                        [&](int r, int j) { return s.C[r * ldd + j]; },
                        [&](int r, int j, double x) { s.Q[r * ldd + j] = x; });
            for (int r = lane; r < d; r += kWave) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < n; ++k) {
                    s1 = fma(s.W[r * ldn + k], s.f[k], s1);
                    s2 = fma(s.F[k * ldd + r], s.v[k], s2);
                }
                s.q[r] = s.c[r] + s1 + s2;
            }
            wsync();
            // [Q_uu | q_u | Q_ux] (in W's place) -> elimination without pivoting -> [I | Q_uu^-1 q_u | Q_uu^-1 Q_ux]
            wave_for_2d(m, s.width, [&](int r, int j, int) {
                double x;
                if (j < m) x = s.Q[(n + r) * ldd + n + j];
                else if (j == m) x = s.q[n + r];
                else x = s.Q[(n + r) * ldd + (j - m - 1)];
                s.aug[r * lda + j] = x;
            });
            wsync();
            if (wave_eliminate_f64(s.aug, lda, m, s.width, s.fac)) status |= TFMPC_ST_NOT_PD;
            wave_for_2d(m, n, [&](int r, int j, int idx) {
                const double x = -s.aug[r * lda + m + 1 + j];
                s.K[r * ldn + j] = x;
                Kg[(size_t)t * m * n + idx] = x;
            });
            for (int r = lane; r < m; r += kWave) {
                const double x = -s.aug[r * lda + m];
                s.k[r] = x;
                kg[(size_t)t * m + r] = x;
            }
            wsync();
            // V' = Q_xx + Q_xu K, over Q_xx ; v' = q_x + Q_xu k  (Schur form)
            wave_matmul_f64<MAXD>(n, n, m,
                        [&](int i, int k) { return s.Q[i * ldd + n + k]; },
                        [&](int k, int j) { return s.K[k * ldn + j]; },
                        [&](int i, int j) { return s.Q[i * ldd + j]; },
                        [&](int i, int j, double x) { s.Q[i * ldd + j] = x; });
            for (int i = lane; i < n; i += kWave) {
                double s1 = 0.0;
                for (int k = 0; k < m; ++k) s1 = fma(s.Q[i * ldd + n + k], s.k[k], s1);
                s.vn[i] = s.q[i] + s1;
            }
            // const += 1/2 k^T Q_uu k + k^T q_u + 1/2 f_t^T V f_t + f_t^T v (V, v before this step's update)
            double part = 0.0;
            for (int r = lane; r < m; r += kWave) {
                double quk = 0.0;
                for (int k = 0; k < m; ++k) quk = fma(s.Q[(n + r) * ldd + n + k], s.k[k], quk);
                part += s.k[r] * (0.5 * quk + s.q[n + r]);
            }
            for (int i = lane; i < n; i += kWave) {
                double vf = 0.0;
                for (int k = 0; k < n; ++k) vf = fma(s.V[i * ldn + k], s.f[k], vf);
                part += s.f[i] * (0.5 * vf + s.v[i]);
            }
            cst += wave_sum_f64(part);
            wsync();
            // V <- (V' + V'^T) / 2: the elimination above reads a symmetric Q_uu only while V stays symmetric
            wave_for_2d(n, n, [&](int i, int j, int idx) {
                const double x = 0.5 * (s.Q[i * ldd + j] + s.Q[j * ldd + i]);
                s.V[i * ldn + j] = x;
                if (a.V) a.V[((size_t)b * T + t) * n * n + idx] = x;
            });
            for (int i = lane; i < n; i += kWave) {
                const double x = s.vn[i];
                s.v[i] = x;
                if (a.v) a.v[((size_t)b * T + t) * n + i] = x;
            }
            if (a.cst && lane == 0) a.cst[(size_t)b * T + t] = cst;
            wsync();
        }
        if (!finite_f64(cst)) status |= TFMPC_ST_NAN;
    }

    if (FORWARD) {
        double *xs = a.states + (size_t)b * (T + 1) * n;
        double *us = a.actions + (size_t)b * T * m;
        double *cs = a.costs + (size_t)b * (T + 1);
        __syncthreads();                                 // gains written above are visible
        for (int i = lane; i < n; i += kWave) {
            const double x = a.x0[(size_t)b * n + i];
            s.z[i] = x;
            xs[i] = x;
        }
        for (int t = 0; t < T; ++t) {
            load_model(t);
            load_matrix_f64(s.K, ldn, Kg + (size_t)t * m * n, m, n);
            for (int r = lane; r < m; r += kWave) s.k[r] = kg[(size_t)t * m + r];
            wsync();
            for (int r = lane; r < m; r += kWave) {        // u = K_t x + k_t
                double u = s.k[r];
                for (int j = 0; j < n; ++j) u = fma(s.K[r * ldn + j], s.z[j], u);
                s.z[n + r] = u;
                us[(size_t)t * m + r] = u;
            }
            wsync();
            double part = 0.0;                             // 1/2 z^T C_t z + c_t^T z
            for (int r = lane; r < d; r += kWave) {
                double cz = 0.0;
                for (int j = 0; j < d; ++j) cz = fma(s.C[r * ldd + j], s.z[j], cz);
                part += s.z[r] * (0.5 * cz + s.c[r]);
            }
            for (int i = lane; i < n; i += kWave) {        // x' = F_t z + f_t
                double x = s.f[i];
                for (int j = 0; j < d; ++j) x = fma(s.F[i * ldd + j], s.z[j], x);
                s.xn[i] = x;
            }
            const double cost = wave_sum_f64(part);
            if (lane == 0) cs[t] = cost;
            wsync();
            for (int i = lane; i < n; i += kWave) {
                const double x = s.xn[i];
                s.z[i] = x;
                xs[(size_t)(t + 1) * n + i] = x;
            }
            wsync();
        }
        double part = 0.0;                                 // 1/2 x^T C_fin x + c_fin^T x
        for (int r = lane; r < n; r += kWave) {
            double cz = 0.0;
            for (int j = 0; j < n; ++j) cz = fma(Cf[r * ldf + j], s.z[j], cz);
            part += s.z[r] * (0.5 * cz + cf[r]);
        }
        const double last_cost = wave_sum_f64(part);
        if (lane == 0) cs[T] = last_cost;
        if (!finite_f64(last_cost)) status |= TFMPC_ST_NAN;
    }

    if (a.status && lane == 0) a.status[b] = status;
}

template <int MAXD, bool BACKWARD, bool FORWARD>
__global__ __launch_bounds__(kWave) void tvlqr_f64_kernel(TvLqrArgsF64 a)
{
    extern __shared__ double smem_f64[];
    tvlqr_f64_body<MAXD, BACKWARD, FORWARD>(a, smem_f64);
}

template <int MAXD, bool BW, bool FW>
int launch(const TvLqrArgsF64 &a, hipStream_t stream)
{
    const size_t smem = tv_smem_doubles(a.n, a.m) * sizeof(double);
    if (smem > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
    auto kern = tvlqr_f64_kernel<MAXD, BW, FW>;
    if (smem > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)smem) != hipSuccess)
            return TFMPC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(a.B), dim3(kWave), smem, stream, a);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

template <int MAXD>
int launch_for(const TvLqrArgsF64 &a, bool backward, bool forward, hipStream_t stream)
{
    if (backward && forward) return launch<MAXD, true, true>(a, stream);
    if (backward) return launch<MAXD, true, false>(a, stream);
    return launch<MAXD, false, true>(a, stream);
}

bool wave16(int n, int m) { return n <= 16 && m <= 16; }

int run(const TvLqrArgsF64 &a, bool bw, bool fw, void *stream)
{
    if (a.B == 0) return TFMPC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return wave16(a.n, a.m) ? launch_for<16>(a, bw, fw, s) : launch_for<32>(a, bw, fw, s);
}

struct ModelF64 {
    const double *F; long sF_b, sF_t;
    const double *f; long sf_b, sf_t;
    const double *C; long sC_b, sC_t;
    const double *c; long sc_b, sc_t;
    const double *Cfin; long sCfin_b;
    const double *cfin; long scfin_b;
};

// the checks of tvlqr_dispatch.hip::check_model, in the same order
int check_model(int B, int n, int m, int T, const ModelF64 &md)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (n > kTvF64MaxDim || m > kTvF64MaxDim) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;                                    // no-op: nothing is read (empty tensors may be NULL)
    if (!md.F || !md.f || !md.C || !md.c) return TFMPC_ERR_ARG;
    if (!md.Cfin != !md.cfin) return TFMPC_ERR_ARG;                 // both or neither
    for (long s : {md.sF_b, md.sF_t, md.sf_b, md.sf_t, md.sC_b, md.sC_t, md.sc_b, md.sc_t, md.sCfin_b, md.scfin_b})
        if (s < 0) return TFMPC_ERR_ARG;
    return TFMPC_OK;
}

TvLqrArgsF64 make_args(int B, int n, int m, int T, const ModelF64 &md)
{
    TvLqrArgsF64 a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = md.F; a.sF_b = md.sF_b; a.sF_t = md.sF_t;
    a.f = md.f; a.sf_b = md.sf_b; a.sf_t = md.sf_t;
    a.C = md.C; a.sC_b = md.sC_b; a.sC_t = md.sC_t;
    a.c = md.c; a.sc_b = md.sc_b; a.sc_t = md.sc_t;
    a.Cfin = md.Cfin; a.sCfin_b = md.sCfin_b;
    a.cfin = md.cfin; a.scfin_b = md.scfin_b;
    return a;
}

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

#define TFMPC_TVLQR_F64_MODEL_PARAMS                                                                                   \
    int B, int n, int m, int T, const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,          \
        const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t, const double *Cfin, long sCfin_b, \
        const double *cfin, long scfin_b
#define TFMPC_TVLQR_F64_MODEL ModelF64{F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b}

extern "C" {

size_t tfmpc_tvlqr_workspace_bytes_f64(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return (size_t)B * T * m * (n + 1) * sizeof(double);
}

const char *tfmpc_tvlqr_kernel_name_f64(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    if (n > kTvF64MaxDim || m > kTvF64MaxDim) return "unsupported";
    return wave16(n, m) ? "tv_f64_wave16" : "tv_f64_wave32";
}

int tfmpc_tvlqr_backward_f64(TFMPC_TVLQR_F64_MODEL_PARAMS, double *K, double *k, double *V, double *v, double *cst,
                             int32_t *status, void *stream)
{
    const ModelF64 md = TFMPC_TVLQR_F64_MODEL;
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (!K || !k) return TFMPC_ERR_ARG;
    TvLqrArgsF64 a = make_args(B, n, m, T, md);
    a.K = K; a.k = k; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v; a.cst = cst; a.status = status;
    return run(a, true, false, stream);
}

int tfmpc_tvlqr_forward_f64(TFMPC_TVLQR_F64_MODEL_PARAMS, const double *K, long strideK, const double *k, long stride_k,
                            const double *x0, double *states, double *actions, double *costs, void *stream)
{
    const ModelF64 md = TFMPC_TVLQR_F64_MODEL;
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (strideK < 0 || stride_k < 0) return TFMPC_ERR_ARG;
    if (!x0 || !states || !costs || !K || !k || !actions) return TFMPC_ERR_ARG;
    TvLqrArgsF64 a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = const_cast<double *>(K); a.k = const_cast<double *>(k); a.sK = strideK; a.sk = stride_k;
    a.states = states; a.actions = actions; a.costs = costs;
    return run(a, false, true, stream);
}

int tfmpc_tvlqr_solve_f64(TFMPC_TVLQR_F64_MODEL_PARAMS, const double *x0, double *states, double *actions, double *costs,
                          double *K, double *k, double *V, double *v, double *cst, int32_t *status,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    const ModelF64 md = TFMPC_TVLQR_F64_MODEL;
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (!x0 || !states || !costs || !actions) return TFMPC_ERR_ARG;
    if (!K || !k) {
        // gains are not a requested output: keep them in caller-provided scratch
        if (!workspace || workspace_bytes < tfmpc_tvlqr_workspace_bytes_f64(B, n, m, T)) return TFMPC_ERR_WORKSPACE;
        double *w = static_cast<double *>(workspace);
        if (!K) K = w;
        if (!k) k = w + (size_t)B * T * m * n;
    }
    TvLqrArgsF64 a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = K; a.k = k; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v; a.cst = cst;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    return run(a, true, true, stream);
}

}  // extern "C"
