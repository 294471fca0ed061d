// tvlqr_elements.h -- the two operators on segment elements as wave-cooperative device functions, for
// the kernels that compose elements outside the time-parallel solve's own condense and stitch (the periodic stitch,
// tvlqr_periodic_f64.hip).  The statements are those of tvlqr_time_parallel_f64.hip's blocks, in their
// order: the same products on v_mfma_f64_16x16x4_f64, the same fma() chains, the same pivoted elimination -- a change
// to either belongs in both files.  (The condense and stitch kernels there keep their own blocks: calling these
// functions from them gave the same statements another register allocation, and their instruction text is pinned,
// DESIGN.md 3.25.)
//
// An element e = (A, b, G, H, h) in LDS: A, G, H with leading dimension odd_ld(n), b and h dense.
//   combine, element 1 before element 2:  [Y_A | Y_G | y_b] = (I + G1 H2)^-1 [A1 | G1 | b1 - G1 h2]
//     A = A2 Y_A, b = A2 y_b + b2, G = G2 + sym(A2 Y_G A2^T), H = H1 + sym(A1^T H2 Y_A), h = h1 + A1^T (h2 + H2 y_b)
//   close, the value (P, p) behind element e:  [M | mu] = (I + P G)^-1 [P A | p + P b];  P_s = H + sym(A^T M),
//     p_s = h + A^T mu
#pragma once

#include <hip/hip_runtime.h>

#include "wave_ops_f64.h"

namespace tfmpc {

struct TvElem {
    double *A, *G, *H, *b, *h;
};

// dst[i] = init(i) + sum_k a(i, k) x[k], a row per lane, k ascending
template <class FA, class FInit>
__device__ __forceinline__ void tv_elem_mv(int rows, int K, FA a, const double *x, FInit init, double *dst)
{
    for (int i = lane_id(); i < rows; i += kWave) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = fma(a(i, k), x[k], s);
        dst[i] = init(i) + s;
    }
}

// e2 <- combine(e1, e2): the result takes e1's A, H, h and e2's G, b, and the pointers are exchanged so that e2 names
// it; e1 then names the buffers that still hold e2's OLD A, H, h (and its own G, b).  T1, T2: n x odd_ld(n); wv: n;
// aug: n x odd_ld(3 n + 1); fac: n.  Returns 1 for a zero pivot in I + G1 H2 (all lanes the same value).
template <class MM>
__device__ __forceinline__ int tv_elem_combine(int n, TvElem &e1, TvElem &e2, double *T1, double *T2, double *wv,
                                               double *aug, double *fac)
{
    const int lane = lane_id();
    const int ldn = odd_ld(n), wY = 3 * n + 1, ldY = odd_ld(wY);
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
    const int singular = wave_gauss_jordan<true>(aug, ldY, n, wY, fac, (double *)nullptr);
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
    tv_elem_mv(n, n, [&](int i, int k) { return e1.A[k * ldn + i]; }, wv, [&](int i) { return e1.h[i]; }, e1.h);
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
    // the result is now (e1.A, e2.G, e1.H, e2.b, e1.h)
    double *x;
    x = e1.A; e1.A = e2.A; e2.A = x;
    x = e1.H; e1.H = e2.H; e2.H = x;
    x = e1.h; e1.h = e2.h; e2.h = x;
    return singular;
}

// (Pv, pv) <- close(e, (Pv, pv)).  T2: n x odd_ld(n); aug: n x odd_ld(2 n + 1); fac: n.  Returns 1 for a zero pivot in
// I + P G.
template <class MM>
__device__ __forceinline__ int tv_elem_close(int n, const TvElem &e, double *Pv, double *pv, double *T2, double *aug,
                                             double *fac)
{
    const int lane = lane_id();
    const int ldn = odd_ld(n), wY = 2 * n + 1, ldY = odd_ld(wY);
    // [I + P G | P A | p + P b] -> [I | M | mu]
    MM::matmul(n, n, n, [&](int i, int k) { return Pv[i * ldn + k]; }, [&](int k, int j) { return e.G[k * ldn + j]; },
               [](int i, int j) { return i == j ? 1.0 : 0.0; }, [&](int i, int j, double v) { aug[i * ldY + j] = v; });
    MM::matmul(n, n, n, [&](int i, int k) { return Pv[i * ldn + k]; }, [&](int k, int j) { return e.A[k * ldn + j]; },
               [](int, int) { return 0.0; }, [&](int i, int j, double v) { aug[i * ldY + n + j] = v; });
    for (int i = lane; i < n; i += kWave) {
        double sum = 0.0;
        for (int k = 0; k < n; ++k) sum = fma(Pv[i * ldn + k], e.b[k], sum);
        aug[i * ldY + 2 * n] = pv[i] + sum;
    }
    wsync();
    const int singular = wave_gauss_jordan<true>(aug, ldY, n, wY, fac, (double *)nullptr);
    // T2 = A^T M ; p = h + A^T mu
    MM::matmul(n, n, n, [&](int i, int k) { return e.A[k * ldn + i]; }, [&](int k, int j) { return aug[k * ldY + n + j]; },
               [](int, int) { return 0.0; }, [&](int i, int j, double v) { T2[i * ldn + j] = v; });
    for (int i = lane; i < n; i += kWave) {
        double sum = 0.0;
        for (int k = 0; k < n; ++k) sum = fma(e.A[k * ldn + i], aug[k * ldY + 2 * n], sum);
        pv[i] = e.h[i] + sum;
    }
    wsync();
    wave_for_2d(n, n, [&](int i, int j, int) { Pv[i * ldn + j] = e.H[i * ldn + j] + 0.5 * (T2[i * ldn + j] + T2[j * ldn + i]); });
    wsync();
    return singular;
}

}  // namespace tfmpc
