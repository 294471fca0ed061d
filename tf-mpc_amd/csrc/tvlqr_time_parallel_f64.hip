// tvlqr_time_parallel_f64.hip -- the condense, stitch and finish kernels of the TIME-PARALLEL double-precision
// time-varying LQR (tfmpc_tvlqr_solve_time_parallel_f64); n <= 32 and m <= 32.  The expand kernel is the
// body of tvlqr_wave.h on a segment (tvlqr_f64.hip); the entry point is in tvlqr_dispatch.hip.
//
// A segment element e = (A, b, G, H, h) stands for the conditional value of a piece of the horizon,
//   V_e(x_s, x_e) = max_lam 1/2 x_s^T H x_s + h^T x_s - 1/2 lam^T G lam + lam^T (x_e - A x_s - b).
// One step (R eliminated WITHOUT pivoting, all right-hand sides at once; a non-positive pivot: TFMPC_ST_NOT_PD):
//   A = A_t - B R^-1 S^T, b = f_t - B R^-1 r, G = sym(B R^-1 B^T), H = sym(Q - S R^-1 S^T), h = q - S R^-1 r.
// Combine, element 1 before element 2 (one PIVOTED solve; a zero pivot: TFMPC_ST_SINGULAR):
//   [Y_A | Y_G | y_b] = (I + G1 H2)^-1 [A1 | G1 | b1 - G1 h2]
//   A = A2 Y_A, b = A2 y_b + b2, G = G2 + sym(A2 Y_G A2^T), H = H1 + sym(A1^T H2 Y_A), h = h1 + A1^T (h2 + H2 y_b).
// Close element e with the value (P, p) behind it: [M | mu] = (I + P G)^-1 [P A | p + P b]; P_s = H + sym(A^T M),
// p_s = h + A^T mu.  Boundary state: x_e = (I + G P)^-1 (A x_s + b - G p).
//
// Waves of different instances share nothing, no kernel uses an atomic, and every reduction has a fixed order: an
// instance's bits depend on neither B nor its position, and repeated calls give identical bits.
#include <hip/hip_runtime.h>

#include "lqr_kernels.h"
#include "tvlqr_kernels.h"
#include "wave_ops_f64.h"

namespace tfmpc {

namespace {

struct Elem {
    double *A, *G, *H, *b, *h;
};

__host__ __device__ constexpr int tp_max(int a, int b) { return a > b ? a : b; }

// LDS of a condense wave, in doubles: F_t f_t C_t c_t, two elements (the step's and the accumulated one), two products,
// one vector, the augmented block (R's m x (m + 2 n + 1) or the combine's n x (3 n + 1)) and the multipliers
__host__ __device__ constexpr size_t condense_smem_elems(int n, int m)
{
    const int d = n + m, ldd = odd_ld(d), ldn = odd_ld(n);
    const size_t aug = (size_t)tp_max(m * odd_ld(m + 2 * n + 1), n * odd_ld(3 * n + 1));
    return (size_t)n * ldd + n + (size_t)d * ldd + d + (size_t)8 * n * ldn + 5 * n + aug + tp_max(n, m);
}

// ... of a stitch wave: one element, the value, one product, the augmented block n x (2 n + 1), multipliers, x
__host__ __device__ constexpr size_t stitch_smem_elems(int n)
{
    return (size_t)5 * n * odd_ld(n) + 5 * n + (size_t)n * odd_ld(2 * n + 1);
}

// 32 KiB at n = 16, m = 8 (five waves per CU), 141.25 KiB at n = m = 32 (one)
static_assert(condense_smem_elems(16, 8) == 4096 && condense_smem_elems(32, 32) == 18080,
              "the LDS size sets the resident waves");

// dst[i] = init(i) + sum_k a(i, k) x[k], a row per lane, k ascending
template <class FA, class FInit>
__device__ __forceinline__ void mv(int rows, int K, FA a, const double *x, FInit init, double *dst)
{
    for (int i = lane_id(); i < rows; i += kWave) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = fma(a(i, k), x[k], s);
        dst[i] = init(i) + s;
    }
}

template <int MAXD>
__global__ __launch_bounds__(kWave) void tvlqr_tp_condense_kernel(TvLqrArgsT<double> a, TvTimeParallel tp)
{
    using MM = WaveF64<MAXD>;
    extern __shared__ double smem_tp[];
    const size_t w = blockIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)tp.segments), seg = (int)blockIdx.x - b * tp.segments;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m;
    const int t0 = seg * tp.len, t1 = a.T - t0 < tp.len ? a.T : t0 + tp.len;
    const int ldd = odd_ld(d), ldn = odd_ld(n), wR = m + 2 * n + 1, ldR = odd_ld(wR), wY = 3 * n + 1, ldY = odd_ld(wY);
    double *p = smem_tp;
    double *F = p; p += n * ldd;
    double *f = p; p += n;
    double *C = p; p += d * ldd;
    double *c = p; p += d;
    Elem e1, e2;                  // the step's element; the accumulated one (steps t + 1 .. t1 - 1)
    auto carve = [&](Elem &e) {
        e.A = p; p += n * ldn;
        e.G = p; p += n * ldn;
        e.H = p; p += n * ldn;
        e.b = p; p += n;
        e.h = p; p += n;
    };
    carve(e1);
    carve(e2);
    double *T1 = p; p += n * ldn;
    double *T2 = p; p += n * ldn;
    double *wv = p; p += n;
    double *aug = p; p += tp_max(m * ldR, n * ldY);
    double *fac = p;
    int status = 0;

    for (int t = t1 - 1; t >= t0; --t) {
        load_matrix(F, ldd, tv_at(a.F, a.sF_b, a.sF_t, b, t), n, d);
        load_matrix(C, ldd, tv_at(a.C, a.sC_b, a.sC_t, b, t), d, d);
        const double *fg = tv_at(a.f, a.sf_b, a.sf_t, b, t), *cg = tv_at(a.c, a.sc_b, a.sc_t, b, t);
        for (int i = lane; i < n; i += kWave) f[i] = fg[i];
        for (int i = lane; i < d; i += kWave) c[i] = cg[i];
        wsync();
        // [R | S^T | r | B^T] -> [I | R^-1 S^T | R^-1 r | R^-1 B^T]
        wave_for_2d(m, wR, [&](int r, int j, int) {
            double x;
            if (j < m) x = C[(n + r) * ldd + n + j];
            else if (j < m + n) x = C[(n + r) * ldd + (j - m)];
            else if (j == m + n) x = c[n + r];
            else x = F[(j - m - n - 1) * ldd + n + r];
            aug[r * ldR + j] = x;
        });
        wsync();
        if (wave_gauss_jordan<false>(aug, ldR, m, wR, fac, (double *)nullptr)) status |= TFMPC_ST_NOT_PD;
        const double *Ks = aug + m, *kr = aug + m + n, *Kb = aug + m + n + 1;
        MM::matmul(n, n, m, [&](int i, int k) { return F[i * ldd + n + k]; }, [&](int k, int j) { return -Ks[k * ldR + j]; },
                   [&](int i, int j) { return F[i * ldd + j]; }, [&](int i, int j, double x) { e1.A[i * ldn + j] = x; });
        MM::matmul(n, n, m, [&](int i, int k) { return F[i * ldd + n + k]; }, [&](int k, int j) { return Kb[k * ldR + j]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double x) { e1.G[i * ldn + j] = x; });
        MM::matmul(n, n, m, [&](int i, int k) { return C[i * ldd + n + k]; }, [&](int k, int j) { return -Ks[k * ldR + j]; },
                   [&](int i, int j) { return C[i * ldd + j]; }, [&](int i, int j, double x) { e1.H[i * ldn + j] = x; });
        for (int i = lane; i < n; i += kWave) {
            double sb = f[i], sh = c[i];
            for (int k = 0; k < m; ++k) {
                const double x = kr[k * ldR];
                sb = fma(-F[i * ldd + n + k], x, sb);
                sh = fma(-C[i * ldd + n + k], x, sh);
            }
            e1.b[i] = sb;
            e1.h[i] = sh;
        }
        wsync();
        symmetrise(e1.G, ldn, n);
        symmetrise(e1.H, ldn, n);
        wsync();
        if (t == t1 - 1) {        // the segment's last step is the first element
            const Elem e = e1;
            e1 = e2;
            e2 = e;
            continue;
        }
        // [I + G1 H2 | A1 | G1 | b1 - G1 h2]
        MM::matmul(n, n, n, [&](int i, int k) { return e1.G[i * ldn + k]; }, [&](int k, int j) { return e2.H[k * ldn + j]; },
                   [](int i, int j) { return i == j ? 1.0 : 0.0; }, [&](int i, int j, double x) { aug[i * ldY + j] = x; });
        wave_for_2d(n, n, [&](int i, int j, int) {
            aug[i * ldY + n + j] = e1.A[i * ldn + j];
            aug[i * ldY + 2 * n + j] = e1.G[i * ldn + j];
        });
        for (int i = lane; i < n; i += kWave) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(e1.G[i * ldn + k], e2.h[k], s);
            aug[i * ldY + 3 * n] = e1.b[i] - s;
        }
        wsync();
        if (wave_gauss_jordan<true>(aug, ldY, n, wY, fac, (double *)nullptr)) status |= TFMPC_ST_SINGULAR;
        const double *YA = aug + n, *YG = aug + 2 * n, *yb = aug + 3 * n;
        // T1 = H2 Y_A ; w = h2 + H2 y_b
        MM::matmul(n, n, n, [&](int i, int k) { return e2.H[i * ldn + k]; }, [&](int k, int j) { return YA[k * ldY + j]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double x) { T1[i * ldn + j] = x; });
        for (int i = lane; i < n; i += kWave) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(e2.H[i * ldn + k], yb[k * ldY], s);
            wv[i] = e2.h[i] + s;
        }
        wsync();
        // T2 = A1^T T1 ; h = h1 + A1^T w (over h1)
        MM::matmul(n, n, n, [&](int i, int k) { return e1.A[k * ldn + i]; }, [&](int k, int j) { return T1[k * ldn + j]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double x) { T2[i * ldn + j] = x; });
        mv(n, n, [&](int i, int k) { return e1.A[k * ldn + i]; }, wv, [&](int i) { return e1.h[i]; }, e1.h);
        wsync();
        // H = H1 + sym(T2) (over H1) ; T1 = A2 Y_G ; b = A2 y_b + b2 (over b2)
        wave_for_2d(n, n, [&](int i, int j, int) { e1.H[i * ldn + j] += 0.5 * (T2[i * ldn + j] + T2[j * ldn + i]); });
        MM::matmul(n, n, n, [&](int i, int k) { return e2.A[i * ldn + k]; }, [&](int k, int j) { return YG[k * ldY + j]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double x) { T1[i * ldn + j] = x; });
        for (int i = lane; i < n; i += kWave) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(e2.A[i * ldn + k], yb[k * ldY], s);
            e2.b[i] = s + e2.b[i];
        }
        wsync();
        // T2 = T1 A2^T
        MM::matmul(n, n, n, [&](int i, int k) { return T1[i * ldn + k]; }, [&](int k, int j) { return e2.A[j * ldn + k]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double x) { T2[i * ldn + j] = x; });
        wsync();
        // G = G2 + sym(T2) (over G2) ; A = A2 Y_A (in A1's place)
        wave_for_2d(n, n, [&](int i, int j, int) { e2.G[i * ldn + j] += 0.5 * (T2[i * ldn + j] + T2[j * ldn + i]); });
        MM::matmul(n, n, n, [&](int i, int k) { return e2.A[i * ldn + k]; }, [&](int k, int j) { return YA[k * ldY + j]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double x) { e1.A[i * ldn + j] = x; });
        wsync();
        // the accumulated element is now (e1.A, e2.G, e1.H, e2.b, e1.h)
        double *x;
        x = e1.A; e1.A = e2.A; e2.A = x;
        x = e1.H; e1.H = e2.H; e2.H = x;
        x = e1.h; e1.h = e2.h; e2.h = x;
    }

    double *out = tp.elems + w * tv_tp_elem_doubles(n);
    store_matrix(out, e2.A, ldn, n, n);
    store_matrix(out + n * n, e2.G, ldn, n, n);
    store_matrix(out + 2 * n * n, e2.H, ldn, n, n);
    for (int i = lane; i < n; i += kWave) {
        out[3 * n * n + i] = e2.b[i];
        out[3 * n * n + n + i] = e2.h[i];
    }
    if (lane == 0) tp.st_condense[w] = status;
}

// One wave per instance: backwards over the summaries, the value function at every segment's end; forwards, the state
// at every segment's start.
template <int MAXD>
__global__ __launch_bounds__(kWave) void tvlqr_tp_stitch_kernel(TvLqrArgsT<double> a, TvTimeParallel tp)
{
    using MM = WaveF64<MAXD>;
    extern __shared__ double smem_tp[];
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, d = n + a.m, P = tp.segments;
    const int ldn = odd_ld(n), wY = 2 * n + 1, ldY = odd_ld(wY);
    double *p = smem_tp;
    double *A = p; p += n * ldn;
    double *G = p; p += n * ldn;
    double *H = p; p += n * ldn;
    double *Pv = p; p += n * ldn;
    double *T2 = p; p += n * ldn;
    double *bv = p; p += n;
    double *hv = p; p += n;
    double *pv = p; p += n;
    double *x = p; p += n;
    double *fac = p; p += n;
    double *aug = p;
    const size_t w0 = (size_t)b * P, ne = tv_tp_elem_doubles(n);
    int status = 0;

    const double *Cf = a.Cfin ? a.Cfin + (size_t)b * a.sCfin_b : tv_at(a.C, a.sC_b, a.sC_t, b, a.T - 1);
    const double *cf = a.Cfin ? a.cfin + (size_t)b * a.scfin_b : tv_at(a.c, a.sc_b, a.sc_t, b, a.T - 1);
    const int ldf = a.Cfin ? n : d;
    wave_for_2d(n, n, [&](int i, int j, int) { Pv[i * ldn + j] = Cf[i * ldf + j]; });
    for (int i = lane; i < n; i += kWave) pv[i] = cf[i];
    wsync();
    for (int s = P - 1; s >= 0; --s) {
        store_matrix(tp.Vend + (w0 + s) * n * n, Pv, ldn, n, n);
        for (int i = lane; i < n; i += kWave) tp.vend[(w0 + s) * n + i] = pv[i];
        if (s == 0) break;
        const double *e = tp.elems + (w0 + s) * ne;
        load_matrix(A, ldn, e, n, n);
        load_matrix(G, ldn, e + n * n, n, n);
        load_matrix(H, ldn, e + 2 * n * n, n, n);
        for (int i = lane; i < n; i += kWave) {
            bv[i] = e[3 * n * n + i];
            hv[i] = e[3 * n * n + n + i];
        }
        wsync();
        // [I + P G | P A | p + P b] -> [I | M | mu]
        MM::matmul(n, n, n, [&](int i, int k) { return Pv[i * ldn + k]; }, [&](int k, int j) { return G[k * ldn + j]; },
                   [](int i, int j) { return i == j ? 1.0 : 0.0; }, [&](int i, int j, double v) { aug[i * ldY + j] = v; });
        MM::matmul(n, n, n, [&](int i, int k) { return Pv[i * ldn + k]; }, [&](int k, int j) { return A[k * ldn + j]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double v) { aug[i * ldY + n + j] = v; });
        for (int i = lane; i < n; i += kWave) {
            double sum = 0.0;
            for (int k = 0; k < n; ++k) sum = fma(Pv[i * ldn + k], bv[k], sum);
            aug[i * ldY + 2 * n] = pv[i] + sum;
        }
        wsync();
        if (wave_gauss_jordan<true>(aug, ldY, n, wY, fac, (double *)nullptr)) status |= TFMPC_ST_SINGULAR;
        // T2 = A^T M ; p = h + A^T mu
        MM::matmul(n, n, n, [&](int i, int k) { return A[k * ldn + i]; }, [&](int k, int j) { return aug[k * ldY + n + j]; },
                   [](int, int) { return 0.0; }, [&](int i, int j, double v) { T2[i * ldn + j] = v; });
        for (int i = lane; i < n; i += kWave) {
            double sum = 0.0;
            for (int k = 0; k < n; ++k) sum = fma(A[k * ldn + i], aug[k * ldY + 2 * n], sum);
            pv[i] = hv[i] + sum;
        }
        wsync();
        wave_for_2d(n, n, [&](int i, int j, int) { Pv[i * ldn + j] = H[i * ldn + j] + 0.5 * (T2[i * ldn + j] + T2[j * ldn + i]); });
        wsync();
    }
    wsync();                                             // the values stored above are read back below

    const int ld1 = odd_ld(n + 1);
    for (int i = lane; i < n; i += kWave) x[i] = a.x0[(size_t)b * n + i];
    wsync();
    for (int s = 0; s < P; ++s) {
        for (int i = lane; i < n; i += kWave) tp.xstart[(w0 + s) * n + i] = x[i];
        if (s == P - 1) break;
        const double *e = tp.elems + (w0 + s) * ne;
        load_matrix(A, ldn, e, n, n);
        load_matrix(G, ldn, e + n * n, n, n);
        load_matrix(Pv, ldn, tp.Vend + (w0 + s) * n * n, n, n);
        for (int i = lane; i < n; i += kWave) {
            bv[i] = e[3 * n * n + i];
            pv[i] = tp.vend[(w0 + s) * n + i];
        }
        wsync();
        // [I + G P | A x + b - G p] -> [I | x']
        MM::matmul(n, n, n, [&](int i, int k) { return G[i * ldn + k]; }, [&](int k, int j) { return Pv[k * ldn + j]; },
                   [](int i, int j) { return i == j ? 1.0 : 0.0; }, [&](int i, int j, double v) { aug[i * ld1 + j] = v; });
        for (int i = lane; i < n; i += kWave) {
            double s1 = 0.0, s2 = 0.0;
            for (int k = 0; k < n; ++k) {
                s1 = fma(A[i * ldn + k], x[k], s1);
                s2 = fma(G[i * ldn + k], pv[k], s2);
            }
            aug[i * ld1 + n] = (s1 + bv[i]) - s2;
        }
        wsync();
        if (wave_gauss_jordan<true>(aug, ld1, n, n + 1, fac, (double *)nullptr)) status |= TFMPC_ST_SINGULAR;
        for (int i = lane; i < n; i += kWave) x[i] = aug[i * ld1 + n];
        wsync();
    }
    if (lane == 0) tp.st_stitch[b] = status;
}

// One wave per instance: the instance's status is the OR over its segments and the stitch; a flagged instance gets NaN
// in its own outputs.
__global__ __launch_bounds__(kWave) void tvlqr_tp_finish_kernel(TvLqrArgsT<double> a, TvTimeParallel tp)
{
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, T = a.T, P = tp.segments;
    const size_t w0 = (size_t)b * P;
    int mine = lane == 0 ? tp.st_stitch[b] : 0;
    for (int s = lane; s < P; s += kWave) mine |= tp.st_condense[w0 + s] | tp.st_expand[w0 + s];
    int status = 0;
    for (int bit = 0; bit < 8; ++bit)
        if (__ballot(mine >> bit & 1)) status |= 1 << bit;
    if (a.status && lane == 0) a.status[b] = status;
    if (status == 0) return;
    auto fill = [&](double *q, size_t per_instance) {
        if (!q) return;
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        q += (size_t)b * per_instance;
        for (size_t i = lane; i < per_instance; i += kWave) q[i] = qnan;
    };
    fill(a.states, (size_t)(T + 1) * n);
    fill(a.actions, (size_t)T * m);
    fill(a.costs, (size_t)T + 1);
    fill(a.K, (size_t)T * m * n);
    fill(a.k, (size_t)T * m);
    fill(a.V, (size_t)T * n * n);
    fill(a.v, (size_t)T * n);
}

template <class K, class... Args>
int launch_waves(K kern, size_t blocks, size_t smem, hipStream_t stream, Args... args)
{
    return launch_with_lds(kern, (unsigned)blocks, kWave, smem, stream, args...);
}

}  // namespace

const char *tvlqr_time_parallel_f64_kernel_name(int n, int m)
{
    return wave16(n, m) ? "tv_f64_time_parallel16" : "tv_f64_time_parallel32";
}

int tvlqr_time_parallel_f64_condense_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream)
{
    const size_t smem = condense_smem_elems(a.n, a.m) * sizeof(double), blocks = (size_t)a.B * tp.segments;
    return wave16(a.n, a.m) ? launch_waves(tvlqr_tp_condense_kernel<16>, blocks, smem, stream, a, tp)
                            : launch_waves(tvlqr_tp_condense_kernel<32>, blocks, smem, stream, a, tp);
}

int tvlqr_time_parallel_f64_stitch_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream)
{
    const size_t smem = stitch_smem_elems(a.n) * sizeof(double);
    return wave16(a.n, a.m) ? launch_waves(tvlqr_tp_stitch_kernel<16>, a.B, smem, stream, a, tp)
                            : launch_waves(tvlqr_tp_stitch_kernel<32>, a.B, smem, stream, a, tp);
}

int tvlqr_time_parallel_f64_finish_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream)
{
    return launch_waves(tvlqr_tp_finish_kernel, a.B, 0, stream, a, tp);
}

}  // namespace tfmpc
