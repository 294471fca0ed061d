// tvlqr_periodic_vjp_f64.hip -- DOUBLE-PRECISION gradients of the PERIODIC infinite-horizon LQR
// (tfmpc_tvlqr_periodic_vjp_f64, include/tfmpc_hip.h): a wrap-around adjoint; n <= 32 and m <= 32.
//
// Given the stationary cycle K_t, k_t, V_t, v_t of one period of N steps (tfmpc_tvlqr_periodic_steady_state_f64) and
// upstream gradients gK, gk, gV, gv, the adjoint of the Riccati recursion is swept FORWARD in time carrying Vbar (n x n,
// symmetric) and vbar (n), the adjoints of V_t and v_t.  The step and its kernel template are
// tvlqr_backward_vjp_body.h's (shared with the finite horizon, tvlqr_backward_vjp_f64.hip).  This file is the PERIODIC
// mode -- abar = 0 (the infinite horizon has no const output), P = V_{(t+1) % N}, s = v_{(t+1) % N}, one wave per
// (instance, segment), three passes that differ in the incoming adjoint and in what they keep -- and what closes the lap.
// The period has no final cost: the adjoint that leaves step N - 1 is the adjoint of V_N = V_0 and re-enters step 0.  One
// lap maps the adjoint (X, y) that enters phase 0 from the wrap to
//   y_out = Phi y + s_y,  X_out = Phi X Phi' + L(y) + S_X,   Phi = A_cl,N-1 ... A_cl,0,  A_cl,t = F_t,x + F_t,u K_t,
// block triangular, so the fixed point takes three sweeps, one n x n solve and one Stein equation.  The sweep is affine
// in the incoming adjoint with the matrix A_cl,t, so the period is cut into P segments (DESIGN.md 3.19's table) that are
// swept concurrently, one wave per (instance, segment).  Launches on the caller's stream (no allocation, no sync, no
// atomics):
//   1. sweep, pass A   from (0, 0): the segment's Psi_s = prod A_cl,t and its outgoing vbar s_s
//   2. stitch A        one wave per instance: Phi = Psi_{P-1} ... Psi_0, s_y; y* = (I - Phi)^-1 s_y by pivoted elimination
//                      (a zero pivot: TFMPC_ST_SINGULAR); y_{s+1} = Psi_s y_s + s_s
//   3. sweep, pass B   from (0, y_s): the outgoing Vbar W_s
//   4. stitch B        W <- Psi_s W Psi_s' + W_s; Smith doubling X <- X + Phi_k X Phi_k', Phi_{k+1} = Phi_k^2 from X = W until
//                      max|Phi_k X Phi_k'| <= tol max(1, max|X|) and max|Phi_{k+1}| <= 1e-3 (a non-finite entry or no stop
//                      within max_iter steps: TFMPC_ST_NOT_STABILISING); X* = sym(X); X_{s+1} = sym(Psi_s X_s Psi_s') + W_s
//   5. sweep, pass C   from (X_s, y_s): writes dF, df, dC, dc and the outgoing adjoint
//   6. finish          ORs the status words, NaN-fills a flagged instance's rows or records, writes the residual: the
//                      distance of the last segment's outgoing adjoint from (X*, y*), relative
//   7. batch sums      batch_sum.h, for every gradient whose batch stride is 0
// A phase does not run on an instance an earlier phase flagged: every stitch hands the OR of all earlier words on.  Waves
// of different instances share nothing and every sum has a fixed order: an instance's bits depend on neither B nor its
// position, and repeated calls give identical bits.  The build is -ffp-contract=off: every fused multiply-add is a
// written fma().
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "../../include/tfmpc_hip.h"
#include "batch_sum.h"
#include "launch.h"
#include "options.h"
#include "tvlqr_backward_vjp_body.h"

namespace tfmpc {

namespace {

constexpr int kRedChunk = 64;          // instances per stage-1 block of the batch sum
constexpr double kSmithPhiZero = 1e-3;
constexpr int kSmithMaxIter = 40;      // DESIGN.md 3.25's defaults
constexpr double kSmithTol = 4.0 * DBL_EPSILON;
constexpr int kOuts = kOutc + 1;       // dF, df, dC, dc

struct PvArgs {
    int B, n, m, N, segments, len;
    const double *F, *f, *C, *c;
    long sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t;
    const double *K, *k, *V, *v;
    const int32_t *fwd_status;
    const double *gK, *gk, *gV, *gv;
    BvOut o[kOuts];
    double *Psi, *Ws, *Xs;             // per (b, segment) [n][n]: prod A_cl; outgoing Vbar of pass B, then C; incoming X
    double *sv, *ys;                   // per (b, segment) [n]: outgoing vbar of pass A, then C; incoming y
    double *Phi;                       // per instance [n][n]: the closed-loop monodromy
    int32_t *st_a, *st_b, *st_c;       // [B segments]: the sweeps' words
    int32_t *st_sa, *st_sb;            // [B]: the stitches' words, each the OR of everything before it
    int max_iter;
    double tol;
    double *residual;                  // [B] or NULL
    int32_t *iterations;               // [B] or NULL
    int32_t *status;
};

// the mode of tvb_vjp_f64_kernel (tvlqr_backward_vjp_body.h): which of the three sweeps
template <int PASS>
struct Periodic {
    using Args = PvArgs;
    static constexpr bool kPeriodic = true;
    static constexpr int kPass = PASS;
    static __device__ int steps(const PvArgs &a) { return a.N; }
};

static_assert(BvLayout<16>::total(kPassA) == 4976 && BvLayout<32>::total(kPassA) == 19168,
              "DESIGN.md 3.26: 38.875 KiB and 149.75 KiB in pass A, 36.75 KiB and 141.5 KiB in passes B and C");

// OR over the lanes of 8-bit status words
__device__ __forceinline__ int wave_or8(int mine)
{
    int status = 0;
    for (int bit = 0; bit < 8; ++bit)
        if (__ballot(mine >> bit & 1)) status |= 1 << bit;
    return status;
}

// LDS of a stitch wave, in doubles: four n x n tiles, the augmented block n x (n + 1), the multipliers, two vectors
__host__ __device__ constexpr size_t stitch_smem_elems(int n)
{
    return (size_t)4 * n * odd_ld(n) + (size_t)n * odd_ld(n + 1) + 3 * n;
}

// One wave per instance.  MODE kPassA: after pass A; kPassB: after pass B.
template <int NP, int MODE>
__global__ __launch_bounds__(kWave) void tvp_vjp_f64_stitch_kernel(PvArgs a)
{
    extern __shared__ double tvp_vjp_stitch_smem_f64[];
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.n, P = a.segments, ldn = odd_ld(n);
    const size_t w0 = (size_t)b * P, nn = (size_t)n * n;
    double *p = tvp_vjp_stitch_smem_f64;
    double *A0 = p; p += n * ldn;
    double *A1 = p; p += n * ldn;
    double *A2 = p; p += n * ldn;
    double *A3 = p; p += n * ldn;
    double *aug = p; p += n * odd_ld(n + 1);
    double *fac = p; p += n;
    double *yc = p; p += n;
    double *yn = p;
    auto zero = [](int, int) { return 0.0; };

    int mine = lane == 0 ? (MODE == kPassA ? a.fwd_status[b] : a.st_sa[b]) : 0;
    const int32_t *words = MODE == kPassA ? a.st_a : a.st_b;
    for (int s = lane; s < P; s += kWave) mine |= words[w0 + s];
    int status = wave_or8(mine);
    int32_t *const word = (MODE == kPassA ? a.st_sa : a.st_sb) + b;
    if (status) {
        if (lane == 0) {
            *word = status;
            if (MODE == kPassB && a.iterations) a.iterations[b] = 0;
        }
        return;
    }

    if (MODE == kPassA) {
        // ---- fold: Phi = Psi_{P-1} ... Psi_0, s_y <- Psi_s s_y + s_s
        double *Mc = A0, *Mn = A1, *Ps = A2;
        load_matrix(Mc, ldn, a.Psi + w0 * nn, n, n);
        for (int i = lane; i < n; i += kWave) yc[i] = a.sv[w0 * n + i];
        lds_sync();
        for (int s = 1; s < P; ++s) {
            load_matrix(Ps, ldn, a.Psi + (w0 + s) * nn, n, n);
            lds_sync();
            wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return Ps[i * ldn + k]; }, [&](int k, int j) { return Mc[k * ldn + j]; },
                                zero, [&](int i, int j, double x) { Mn[i * ldn + j] = x; });
            wave_matvec<double>(n, n, [&](int i, int k) { return Ps[i * ldn + k]; }, [&](int k) { return yc[k]; },
                                [&](int i, double x) { yn[i] = x + a.sv[(w0 + s) * n + i]; });
            lds_sync();
            double *x;
            x = Mc; Mc = Mn; Mn = x;
            x = yc; yc = yn; yn = x;
        }
        store_matrix(a.Phi + (size_t)b * nn, Mc, ldn, n, n);
        // ---- y* = (I - Phi)^-1 s_y
        const int ldY = odd_ld(n + 1);
        wave_for_2d(n, n + 1, [&](int i, int j, int) {
            aug[i * ldY + j] = j == n ? yc[i] : (i == j ? 1.0 : 0.0) - Mc[i * ldn + j];
        });
        wsync();
        if (wave_gauss_jordan<true>(aug, ldY, n, n + 1, fac, (double *)nullptr)) status |= TFMPC_ST_SINGULAR;
        // ---- y at every segment's start: y_{s+1} = Psi_s y_s + s_s
        bool bad = false;
        for (int i = lane; i < n; i += kWave) yc[i] = aug[i * ldY + n];
        lds_sync();
        for (int s = 0; s < P && !status; ++s) {
            for (int i = lane; i < n; i += kWave) {
                a.ys[(w0 + s) * n + i] = yc[i];
                bad |= !finite(yc[i]);
            }
            if (s == P - 1) break;
            const double *Pg = a.Psi + (w0 + s) * nn;
            wave_matvec<double>(n, n, [&](int i, int k) { return Pg[i * n + k]; }, [&](int k) { return yc[k]; },
                                [&](int i, double x) { yn[i] = x + a.sv[(w0 + s) * n + i]; });
            lds_sync();
            double *x = yc; yc = yn; yn = x;
        }
        if (__ballot(bad)) status |= TFMPC_ST_NAN;
    } else {
        // ---- fold: W <- Psi_s W Psi_s' + W_s
        double *X = A0, *Fk = A1, *T1 = A2, *T2 = A3;
        load_matrix(X, ldn, a.Ws + w0 * nn, n, n);
        lds_sync();
        for (int s = 1; s < P; ++s) {
            const double *Wg = a.Ws + (w0 + s) * nn;
            load_matrix(Fk, ldn, a.Psi + (w0 + s) * nn, n, n);
            lds_sync();
            wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return Fk[i * ldn + k]; }, [&](int k, int j) { return X[k * ldn + j]; },
                                zero, [&](int i, int j, double x) { T1[i * ldn + j] = x; });
            lds_sync();
            wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return T1[i * ldn + k]; }, [&](int k, int j) { return Fk[j * ldn + k]; },
                                [&](int i, int j) { return Wg[i * n + j]; }, [&](int i, int j, double x) { X[i * ldn + j] = x; });
            lds_sync();
        }
        // ---- Smith doubling: X <- X + Phi_k X Phi_k', Phi_{k+1} = Phi_k^2
        load_matrix(Fk, ldn, a.Phi + (size_t)b * nn, n, n);
        lds_sync();
        int it = 0;
        bool converged = false;
        while (it < a.max_iter) {
            ++it;
            double inc = 0.0, Xmax = 0.0, Fmax = 0.0;
            bool bad = false;          // (the maximum drops a NaN operand: non-finite entries are counted on their own)
            wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return Fk[i * ldn + k]; }, [&](int k, int j) { return X[k * ldn + j]; },
                                zero, [&](int i, int j, double x) { T1[i * ldn + j] = x; });
            lds_sync();
            wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return T1[i * ldn + k]; }, [&](int k, int j) { return Fk[j * ldn + k]; },
                                zero, [&](int i, int j, double x) { T2[i * ldn + j] = x; });
            lds_sync();
            wave_for_2d(n, n, [&](int i, int j, int) {
                const double dx = T2[i * ldn + j], xn = X[i * ldn + j] + dx;
                X[i * ldn + j] = xn;
                bad |= !(finite(dx) && finite(xn));
                inc = fmax(inc, fabs(dx));
                Xmax = fmax(Xmax, fabs(xn));
            });
            wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return Fk[i * ldn + k]; }, [&](int k, int j) { return Fk[k * ldn + j]; },
                                zero, [&](int i, int j, double x) {
                                    T1[i * ldn + j] = x;
                                    bad |= !finite(x);
                                    Fmax = fmax(Fmax, fabs(x));
                                });
            const bool nonfinite = __ballot(bad) != 0;
            inc = wave_max(inc);
            Xmax = wave_max(Xmax);
            Fmax = wave_max(Fmax);
            lds_sync();
            double *x = Fk; Fk = T1; T1 = x;
            if (nonfinite) break;
            if (inc <= a.tol * fmax(1.0, Xmax) && Fmax <= kSmithPhiZero) {
                converged = true;
                break;
            }
        }
        if (!converged) status |= TFMPC_ST_NOT_STABILISING;
        if (lane == 0 && a.iterations) a.iterations[b] = it;
        // ---- X at every segment's start: X_0 = X* = sym(X), X_{s+1} = sym(Psi_s X_s Psi_s') + W_s
        if (!status) {
            symmetrise(X, ldn, n);
            lds_sync();
            for (int s = 0; s < P; ++s) {
                store_matrix(a.Xs + (w0 + s) * nn, X, ldn, n, n);
                if (s == P - 1) break;
                const double *Wg = a.Ws + (w0 + s) * nn;
                load_matrix(Fk, ldn, a.Psi + (w0 + s) * nn, n, n);
                lds_sync();
                wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return Fk[i * ldn + k]; }, [&](int k, int j) { return X[k * ldn + j]; },
                                    zero, [&](int i, int j, double x) { T1[i * ldn + j] = x; });
                lds_sync();
                wave_matmul_f64<NP>(n, n, n, [&](int i, int k) { return T1[i * ldn + k]; }, [&](int k, int j) { return Fk[j * ldn + k]; },
                                    zero, [&](int i, int j, double x) { T2[i * ldn + j] = x; });
                lds_sync();
                wave_for_2d(n, n, [&](int i, int j, int) {
                    X[i * ldn + j] = 0.5 * (T2[i * ldn + j] + T2[j * ldn + i]) + Wg[i * n + j];
                });
                lds_sync();
            }
        }
    }
    if (lane == 0) *word = status;
}

// One wave per instance: the status is the OR of stitch B's word (which carries everything before it) and pass C's; a
// non-finite outgoing adjoint is TFMPC_ST_NAN.  A flagged instance gets NaN in its own rows (or records); the others the
// residual.
__global__ __launch_bounds__(kWave) void tvp_vjp_f64_finish_kernel(PvArgs a)
{
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.n, m = a.m, N = a.N, P = a.segments, d = n + m;
    const size_t w0 = (size_t)b * P, nn = (size_t)n * n;
    int mine = lane == 0 ? a.st_sb[b] : 0;
    for (int s = lane; s < P; s += kWave) mine |= a.st_c[w0 + s];
    int status = wave_or8(mine);
    double residual = __builtin_nan("");
    if (!status) {
        const double *Xo = a.Ws + (w0 + P - 1) * nn, *yo = a.sv + (w0 + P - 1) * n, *X0 = a.Xs + w0 * nn, *y0 = a.ys + w0 * n;
        double dX = 0.0, Xmax = 0.0, dy = 0.0, ymax = 0.0;
        bool bad = false;
        for (size_t i = lane; i < nn; i += kWave) {
            bad |= !finite(Xo[i]);
            dX = fmax(dX, fabs(Xo[i] - X0[i]));
            Xmax = fmax(Xmax, fabs(X0[i]));
        }
        for (int i = lane; i < n; i += kWave) {
            bad |= !finite(yo[i]);
            dy = fmax(dy, fabs(yo[i] - y0[i]));
            ymax = fmax(ymax, fabs(y0[i]));
        }
        if (__ballot(bad)) status |= TFMPC_ST_NAN;
        dX = wave_max(dX);
        Xmax = wave_max(Xmax);
        dy = wave_max(dy);
        ymax = wave_max(ymax);
        residual = fmax(dX / fmax(1.0, Xmax), dy / fmax(1.0, ymax));
    }
    if (lane == 0) {
        a.status[b] = status;
        if (a.residual) a.residual[b] = status ? __builtin_nan("") : residual;
    }
    if (!status) return;
    const int sizes[kOuts] = {n * d, n, d * d, d};
    for (int q = 0; q < kOuts; ++q) {
        const BvOut &o = a.o[q];
        if (!o.p) continue;
        const int slots = o.st ? N : 1;
        for (int t = 0; t < slots; ++t) fill_nan(o.p + (size_t)b * o.sb + (size_t)t * o.st, sizes[q]);
    }
}

bool shape_supported(int n, int m) { return n <= 32 && m <= 32; }

size_t up64(size_t x) { return (x + 63) / 64 * 64; }

struct SegmentTable { int len, count; };

// DESIGN.md 3.19's table: `segments` clamped to N, len = ceil(N / segments), count = ceil(N / len)
SegmentTable segment_table(int N, int segments)
{
    if (segments > N) segments = N;
    const long len = ((long)N + segments - 1) / segments;
    return {(int)len, (int)((N + len - 1) / len)};
}

BatchSumPlan sum_plan(int B, int n, int m, const int slots[kOuts], unsigned summed)
{
    const int d = n + m;
    const int sizes[kOuts] = {n * d, n, d * d, d};
    return batch_sum_plan(B, kRedChunk, kOuts, sizes, slots, summed);
}

// The workspace, in doubles: with w = B P, Psi, Ws, Xs (w n n each, rounded up to 64), sv, ys (w n each), Phi (B n n);
// then the batch sum's records and partial sums (batch_sum.h); then the 3 w + 2 B status words.
struct Layout {
    size_t Psi, Ws, Xs, sv, ys, Phi, sum, st, total;
};

Layout layout(int B, int n, int count, size_t sum_doubles)
{
    Layout L{};
    const size_t w = (size_t)B * count;
    size_t o = 0;
    L.Psi = o; o += up64(w * n * n);
    L.Ws = o; o += up64(w * n * n);
    L.Xs = o; o += up64(w * n * n);
    L.sv = o; o += up64(w * n);
    L.ys = o; o += up64(w * n);
    L.Phi = o; o += up64((size_t)B * n * n);
    L.sum = o; o += sum_doubles;
    L.st = o; o += up64((3 * w + 2 * (size_t)B + 1) / 2);                  // 32-bit words
    L.total = o;
    return L;
}

template <int NP, int PASS>
int sweep_for(const PvArgs &a, hipStream_t stream)
{
    return launch_with_lds(tvb_vjp_f64_kernel<NP, Periodic<PASS>>, (unsigned)((size_t)a.B * a.segments), kWave,
                           BvLayout<NP>::total(PASS) * sizeof(double), stream, a);
}

template <int PASS>
int sweep(const PvArgs &a, hipStream_t stream)
{
    return wave16(a.n, a.m) ? sweep_for<16, PASS>(a, stream) : sweep_for<32, PASS>(a, stream);
}

template <int MODE>
int stitch(const PvArgs &a, hipStream_t stream)
{
    const size_t smem = stitch_smem_elems(a.n) * sizeof(double);
    return wave16(a.n, a.m) ? launch_with_lds(tvp_vjp_f64_stitch_kernel<16, MODE>, (unsigned)a.B, kWave, smem, stream, a)
                            : launch_with_lds(tvp_vjp_f64_stitch_kernel<32, MODE>, (unsigned)a.B, kWave, smem, stream, a);
}

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

size_t tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(int B, int n, int m, int N, int segments)
{
    if (B <= 0 || n <= 0 || m <= 0 || N <= 0 || segments < 1 || !shape_supported(n, m)) return 0;
    const int slots[kOuts] = {N, N, N, N};
    const size_t sum = B > 1 ? sum_plan(B, n, m, slots, (1u << kOuts) - 1).floats : 0;
    return layout(B, n, segment_table(N, segments).count, sum).total * sizeof(double);
}

const char *tfmpc_tvlqr_periodic_vjp_kernel_name_f64(int n, int m, int N, int segments)
{
    if (n <= 0 || m <= 0 || N <= 0 || segments < 1) return "invalid";
    if (wave16(n, m)) return "tvp_vjp_f64_wave16";
    if (shape_supported(n, m)) return "tvp_vjp_f64_wave32";
    return "unsupported";
}

int tfmpc_tvlqr_periodic_vjp_f64(int B, int n, int m, int N,
                                 const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                                 const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                                 const double *K, const double *k, const double *V, const double *v, const int32_t *fwd_status,
                                 const double *gK, const double *gk, const double *gV, const double *gv,
                                 double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                                 double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t,
                                 double *residual, int32_t *iterations, int32_t *status, int segments, int max_iter, double tol,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || N <= 0) return TFMPC_ERR_ARG;
    if (!shape_supported(n, m)) return TFMPC_ERR_UNSUPPORTED;
    if (segments < 1 || max_iter < 0 || !(tol >= 0.0)) return TFMPC_ERR_ARG;
    if (B == 0) return TFMPC_OK;
    if (!F || !f || !C || !c || !K || !k || !V || !v || !fwd_status || !status) return TFMPC_ERR_ARG;
    for (long s : {sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t, sdF_b, sdF_t, sdf_b, sdf_t, sdC_b, sdC_t, sdc_b, sdc_t})
        if (s < 0) return TFMPC_ERR_ARG;
    double *outs[kOuts] = {dF, df, dC, dc};
    const long sb[kOuts] = {sdF_b, sdf_b, sdC_b, sdc_b};
    const long st[kOuts] = {sdF_t, sdf_t, sdC_t, sdc_t};
    // a batch stride of 0 sums over the batch (over a batch of one the sum is the instance's own gradient, written in
    // place); a time stride of 0 sums over time in the sweep, in time order: the period is then ONE segment
    int slots[kOuts];
    const unsigned summed = batch_sum_select(B, kOuts, outs, sb, st, N, slots);
    bool time_shared = false;
    for (int q = 0; q < kOuts; ++q)
        if (outs[q] && st[q] == 0 && N > 1) time_shared = true;
    const SegmentTable tab = segment_table(N, time_shared ? 1 : segments);
    if ((size_t)B * tab.count > (size_t)INT32_MAX) return TFMPC_ERR_UNSUPPORTED;
    const BatchSumPlan plan = sum_plan(B, n, m, slots, summed);
    if (!plan.fits) return TFMPC_ERR_UNSUPPORTED;                  // the batch sum's blocks are one grid axis
    const Layout L = layout(B, n, tab.count, plan.floats);
    if (!workspace || workspace_bytes < L.total * sizeof(double)) return TFMPC_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(double)) return TFMPC_ERR_ARG;      // doubles are carved from it
    double *w = static_cast<double *>(workspace);

    PvArgs a{};
    a.B = B; a.n = n; a.m = m; a.N = N; a.segments = tab.count; a.len = tab.len;
    a.F = F; a.f = f; a.C = C; a.c = c;
    a.sF_b = sF_b; a.sF_t = sF_t; a.sf_b = sf_b; a.sf_t = sf_t; a.sC_b = sC_b; a.sC_t = sC_t; a.sc_b = sc_b; a.sc_t = sc_t;
    a.K = K; a.k = k; a.V = V; a.v = v; a.fwd_status = fwd_status;
    a.gK = gK; a.gk = gk; a.gV = gV; a.gv = gv;
    double *const sums = w + L.sum;
    batch_sum_route(plan, sums, outs, sb, st, [&](int q, double *p, long b, long t) { a.o[q] = {p, b, t}; });
    a.Psi = w + L.Psi; a.Ws = w + L.Ws; a.Xs = w + L.Xs; a.sv = w + L.sv; a.ys = w + L.ys; a.Phi = w + L.Phi;
    const size_t waves = (size_t)B * tab.count;
    int32_t *words = reinterpret_cast<int32_t *>(w + L.st);
    a.st_a = words; a.st_b = words + waves; a.st_c = words + 2 * waves;
    a.st_sa = words + 3 * waves; a.st_sb = a.st_sa + B;
    a.max_iter = max_iter ? max_iter : kSmithMaxIter;
    a.tol = tol > 0.0 ? tol : kSmithTol;
    a.residual = residual; a.iterations = iterations; a.status = status;

    // TFMPC_TVLQR_TP_PHASES = 1 .. 5: stop after pass A / stitch A / pass B / stitch B / pass C -- for the phase split of
    // tools/tvlqr_periodic_grad_rate.py only; the outputs are not complete, and the call says so
    const int phases = option_int(kOptTvlqrTpPhases, 6);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if ((rc = sweep<kPassA>(a, s)) != TFMPC_OK) return rc;
    if (phases == 1) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = stitch<kPassA>(a, s)) != TFMPC_OK) return rc;
    if (phases == 2) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = sweep<kPassB>(a, s)) != TFMPC_OK) return rc;
    if (phases == 3) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = stitch<kPassB>(a, s)) != TFMPC_OK) return rc;
    if (phases == 4) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = sweep<kPassC>(a, s)) != TFMPC_OK) return rc;
    if (phases == 5) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = launch_with_lds(tvp_vjp_f64_finish_kernel, (unsigned)B, kWave, 0, s, a)) != TFMPC_OK) return rc;
    return batch_sum_run<kRedChunk, kSumTree, double>(plan, sums, outs, st, s);
}

}  // extern "C"
