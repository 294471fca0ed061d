// tvlqr_periodic_f64.hip -- the stitch and finish kernels of the PERIODIC infinite-horizon LQR in double
// (tfmpc_tvlqr_periodic_steady_state_f64); n <= 32 and m <= 32.  The condense kernel is the time-parallel
// solve's own (tvlqr_time_parallel_f64.hip) on one period, the expand kernel the body of tvlqr_wave.h on a segment without
// a rollout (tvlqr_f64.hip); the entry point is in tvlqr_dispatch.hip.
//
// One wave per instance.  The P segment elements of the period are folded, serially from the last, into the one-period
// element E1 = (A1, b1, G1, H1, h1), which is kept in the workspace.  Doubling, E <- combine(E, E), gives the element of
// 2^k periods: H_k -> P_0 and h_k -> p_0, the periodic stabilising value function at phase 0, while A_k -> 0.  It stops
// after step k when
//   max|H_k - H_{k-1}| <= tol max|H_k|,  max|h_k - h_{k-1}| <= tol max(1, max|h_k|)  and  max|A_k| <= 1e-3;
// a non-finite entry or no stop within max_iter steps is TFMPC_ST_NOT_STABILISING.  The certificate is taken on the
// result: the closed-loop monodromy Phi = (I + G1 P_0)^-1 A1 is squared until max|Phi^(2^j)| <= 1e-3, within max_iter
// squarings (A_k -> 0 alone does not prove stability).  Then (P_0, p_0) is the value behind the LAST
// segment, `close` carries it backwards over segments P - 1 .. 1 to every segment's end, and one more close over segment
// 0 returns to phase 0: its distance from (P_0, p_0) is the residual the caller can read.
//
// Waves of different instances share nothing, no kernel uses an atomic, and every reduction has a fixed order: an
// instance's bits depend on neither B nor its position, and repeated calls give identical bits.
#include <hip/hip_runtime.h>

#include <limits>

#include "lqr_kernels.h"
#include "tvlqr_elements.h"
#include "tvlqr_kernels.h"

namespace tfmpc {

namespace {

constexpr double kPeriodicAZero = 1e-3;

// LDS of a periodic stitch wave, in doubles: two elements, two products, one vector, the combine's augmented block
// n x (3 n + 1) and the multipliers
__host__ __device__ constexpr size_t periodic_stitch_smem_elems(int n)
{
    return (size_t)8 * n * odd_ld(n) + 5 * n + (size_t)n * odd_ld(3 * n + 1) + n;
}

// 23.875 KiB at n = 16 (six waves per CU), 91.75 KiB at n = 32 (one)
static_assert(periodic_stitch_smem_elems(16) == 3056 && periodic_stitch_smem_elems(32) == 11744,
              "the LDS size sets the resident waves");

__device__ __forceinline__ void load_elem(const TvElem &e, const double *g, int n)
{
    const int ldn = odd_ld(n);
    load_matrix(e.A, ldn, g, n, n);
    load_matrix(e.G, ldn, g + n * n, n, n);
    load_matrix(e.H, ldn, g + 2 * n * n, n, n);
    for (int i = lane_id(); i < n; i += kWave) {
        e.b[i] = g[3 * n * n + i];
        e.h[i] = g[3 * n * n + n + i];
    }
}

template <int MAXD>
__global__ __launch_bounds__(kWave) void tvlqr_periodic_stitch_kernel(TvLqrArgsT<double> a, TvTimeParallel tp, TvPeriodic pp)
{
    using MM = WaveF64<MAXD>;
    extern __shared__ double smem_periodic[];
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, P = tp.segments;
    const int ldn = odd_ld(n), ldY = odd_ld(3 * n + 1);
    const size_t w0 = (size_t)b * P, ne = tv_tp_elem_doubles(n);

    // an instance whose condense is flagged: nothing to stitch (the finish kernel fills its outputs)
    int flagged = 0;
    for (int s = lane; s < P; s += kWave) flagged |= tp.st_condense[w0 + s];
    if (__ballot(flagged != 0)) {
        if (lane == 0) {
            tp.st_stitch[b] = 0;
            if (pp.iterations) pp.iterations[b] = 0;
        }
        return;
    }

    double *p = smem_periodic;
    TvElem e1, e2;
    auto carve = [&](TvElem &e) {
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
    double *aug = p; p += n * ldY;
    double *fac = p;
    int status = 0, it = 0;

    // ---- fold: E1 = e_0 (e_1 (... e_{P-1}))
    load_elem(e2, tp.elems + (w0 + P - 1) * ne, n);
    wsync();
    for (int s = P - 2; s >= 0; --s) {
        load_elem(e1, tp.elems + (w0 + s) * ne, n);
        wsync();
        if (tv_elem_combine<MM>(n, e1, e2, T1, T2, wv, aug, fac)) status |= TFMPC_ST_SINGULAR;
    }
    double *E1 = pp.E1 + (size_t)b * ne;
    store_matrix(E1, e2.A, ldn, n, n);
    store_matrix(E1 + n * n, e2.G, ldn, n, n);
    store_matrix(E1 + 2 * n * n, e2.H, ldn, n, n);
    for (int i = lane; i < n; i += kWave) {
        E1[3 * n * n + i] = e2.b[i];
        E1[3 * n * n + n + i] = e2.h[i];
    }

    // ---- double: e2 is E_k; e1 its second copy, and after the combine the step before
    bool converged = false;
    while (!status && it < pp.max_iter) {
        ++it;
        wave_for_2d(n, n, [&](int i, int j, int) {
            e1.A[i * ldn + j] = e2.A[i * ldn + j];
            e1.G[i * ldn + j] = e2.G[i * ldn + j];
            e1.H[i * ldn + j] = e2.H[i * ldn + j];
        });
        for (int i = lane; i < n; i += kWave) {
            e1.b[i] = e2.b[i];
            e1.h[i] = e2.h[i];
        }
        wsync();
        if (tv_elem_combine<MM>(n, e1, e2, T1, T2, wv, aug, fac)) {
            status |= TFMPC_ST_SINGULAR;
            break;
        }
        double dH = 0.0, Hmax = 0.0, Amax = 0.0, dh = 0.0, hmax = 0.0;
        bool bad = false;              // (the maximum drops a NaN operand: non-finite entries are counted on their own)
        wave_for_2d(n, n, [&](int i, int j, int) {
            const double hn = e2.H[i * ldn + j], an = e2.A[i * ldn + j], gn = e2.G[i * ldn + j];
            const double inc = hn - e1.H[i * ldn + j];
            bad |= !(finite(hn) && finite(an) && finite(gn) && finite(inc));
            dH = fmax(dH, fabs(inc));
            Hmax = fmax(Hmax, fabs(hn));
            Amax = fmax(Amax, fabs(an));
        });
        for (int i = lane; i < n; i += kWave) {
            const double hn = e2.h[i], inc = hn - e1.h[i];
            bad |= !(finite(hn) && finite(e2.b[i]) && finite(inc));
            dh = fmax(dh, fabs(inc));
            hmax = fmax(hmax, fabs(hn));
        }
        const bool nonfinite = __ballot(bad) != 0;
        dH = wave_max(dH);
        Hmax = wave_max(Hmax);
        Amax = wave_max(Amax);
        dh = wave_max(dh);
        hmax = wave_max(hmax);
        wsync();
        if (nonfinite) break;
        if (dH <= pp.tol * Hmax && dh <= pp.tol * fmax(1.0, hmax) && Amax <= kPeriodicAZero) {
            converged = true;
            break;
        }
    }
    if (!status && !converged) status |= TFMPC_ST_NOT_STABILISING;

    // (P_0, p_0) = (e2.H, e2.h) from here on; e2.A, e2.b become the travelling value, e1 the element at hand
    double *P0 = e2.H, *p0 = e2.h, *Pv = e2.A, *pv = e2.b;

    // ---- certificate: Phi = (I + G1 P_0)^-1 A1, squared (E1's A and G read back from the workspace into e1)
    if (!status) {
        wsync();                                         // E1 stored above is read back below
        load_matrix(e1.A, ldn, E1, n, n);
        load_matrix(e1.G, ldn, E1 + n * n, n, n);
        wsync();
        const int ld2 = odd_ld(2 * n);
        MM::matmul(n, n, n, [&](int i, int k) { return e1.G[i * ldn + k]; }, [&](int k, int j) { return P0[k * ldn + j]; },
                   [](int i, int j) { return i == j ? 1.0 : 0.0; }, [&](int i, int j, double x) { aug[i * ld2 + j] = x; });
        wave_for_2d(n, n, [&](int i, int j, int) { aug[i * ld2 + n + j] = e1.A[i * ldn + j]; });
        wsync();
        if (wave_gauss_jordan<true>(aug, ld2, n, 2 * n, fac, (double *)nullptr)) status |= TFMPC_ST_SINGULAR;
        wave_for_2d(n, n, [&](int i, int j, int) { T1[i * ldn + j] = aug[i * ld2 + n + j]; });
        wsync();
        bool certified = false;
        for (int j = 0; j < pp.max_iter && !certified && !status; ++j) {      // squares ping-pong between T1 and T2
            double *src = (j & 1) ? T2 : T1, *dst = (j & 1) ? T1 : T2;
            double mx = 0.0;
            bool nf = false;
            MM::matmul(n, n, n, [&](int i, int k) { return src[i * ldn + k]; }, [&](int k, int c2) { return src[k * ldn + c2]; },
                       [](int, int) { return 0.0; }, [&](int i, int c2, double x) {
                           dst[i * ldn + c2] = x;
                           nf |= !finite(x);
                           mx = fmax(mx, fabs(x));
                       });
            if (__ballot(nf)) break;
            certified = wave_max(mx) <= kPeriodicAZero;
            wsync();
        }
        if (!status && !certified) status |= TFMPC_ST_NOT_STABILISING;
    }

    // ---- seams: the value behind every segment, backwards from (P_0, p_0) behind the last; then once more over
    // segment 0, back to phase 0
    double residual = __builtin_nan("");
    if (!status) {
        wsync();
        wave_for_2d(n, n, [&](int i, int j, int) { Pv[i * ldn + j] = P0[i * ldn + j]; });
        for (int i = lane; i < n; i += kWave) pv[i] = p0[i];
        wsync();
        for (int s = P - 1; s >= 0; --s) {
            store_matrix(tp.Vend + (w0 + s) * n * n, Pv, ldn, n, n);
            for (int i = lane; i < n; i += kWave) tp.vend[(w0 + s) * n + i] = pv[i];
            load_elem(e1, tp.elems + (w0 + s) * ne, n);
            wsync();
            if (tv_elem_close<MM>(n, e1, Pv, pv, T2, aug, fac)) status |= TFMPC_ST_SINGULAR;
        }
        double dP = 0.0, Pmax = 0.0, dp = 0.0, pmax = 0.0;
        wave_for_2d(n, n, [&](int i, int j, int) {
            dP = fmax(dP, fabs(Pv[i * ldn + j] - P0[i * ldn + j]));
            Pmax = fmax(Pmax, fabs(P0[i * ldn + j]));
        });
        for (int i = lane; i < n; i += kWave) {
            dp = fmax(dp, fabs(pv[i] - p0[i]));
            pmax = fmax(pmax, fabs(p0[i]));
        }
        dP = wave_max(dP);
        Pmax = wave_max(Pmax);
        dp = wave_max(dp);
        pmax = wave_max(pmax);
        residual = fmax(dP / Pmax, dp / fmax(1.0, pmax));
    }
    if (lane == 0) {
        tp.st_stitch[b] = status;
        if (pp.iterations) pp.iterations[b] = it;
        if (pp.residual) pp.residual[b] = status ? __builtin_nan("") : residual;
    }
}

// One wave per instance: the instance's status is the OR over its segments' condense and expand words and its stitch
// word; a flagged instance gets NaN in its own outputs.  (An expand wave of an instance that condense or stitch flagged
// does not run, and a stitch wave of an instance that condense flagged does not: their words are zero.)
__global__ __launch_bounds__(kWave) void tvlqr_periodic_finish_kernel(TvLqrArgsT<double> a, TvTimeParallel tp, TvPeriodic pp)
{
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, N = a.T, P = tp.segments;
    const size_t w0 = (size_t)b * P;
    int mine = lane == 0 ? tp.st_stitch[b] : 0;
    for (int s = lane; s < P; s += kWave) mine |= tp.st_condense[w0 + s] | tp.st_expand[w0 + s];
    int status = 0;
    for (int bit = 0; bit < 8; ++bit)
        if (__ballot(mine >> bit & 1)) status |= 1 << bit;
    if (lane == 0) a.status[b] = status;
    if (status == 0) return;
    auto fill = [&](double *q, size_t per_instance) {
        if (!q) return;
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        q += (size_t)b * per_instance;
        for (size_t i = lane; i < per_instance; i += kWave) q[i] = qnan;
    };
    fill(a.K, (size_t)N * m * n);
    fill(a.k, (size_t)N * m);
    fill(a.V, (size_t)N * n * n);
    fill(a.v, (size_t)N * n);
    fill(pp.residual, 1);
}

}  // namespace

const char *tvlqr_periodic_f64_kernel_name(int n, int m) { return wave16(n, m) ? "tv_f64_periodic16" : "tv_f64_periodic32"; }

int tvlqr_periodic_f64_stitch_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, const TvPeriodic &pp,
                                     hipStream_t stream)
{
    const size_t smem = periodic_stitch_smem_elems(a.n) * sizeof(double);
    return wave16(a.n, a.m) ? launch_with_lds(tvlqr_periodic_stitch_kernel<16>, (unsigned)a.B, kWave, smem, stream, a, tp, pp)
                            : launch_with_lds(tvlqr_periodic_stitch_kernel<32>, (unsigned)a.B, kWave, smem, stream, a, tp, pp);
}

int tvlqr_periodic_f64_finish_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, const TvPeriodic &pp,
                                     hipStream_t stream)
{
    return launch_with_lds(tvlqr_periodic_finish_kernel, (unsigned)a.B, kWave, 0, stream, a, tp, pp);
}

}  // namespace tfmpc
