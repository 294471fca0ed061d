// lqr_steady_state_f64.hip -- DOUBLE-PRECISION infinite-horizon batched LQR (tfmpc_lqr_steady_state_f64,
// include/tfmpc_hip.h): one wavefront per instance, every matrix in the wave's LDS slice, n <= 32 and
// m <= 32.
//
// The sequence of lqr_steady_state.hip, statement for statement, in double -- a change to either
// recursion belongs in both files.  (One templated body for both was built and measured: it keeps every bit, and the
// fp32 kernels run 2 % slower from it: DESIGN.md 3.16.)  P comes from the structure-preserving doubling algorithm (SDA):
//   A_0 = A - B R^-1 S',  G_0 = B R^-1 B',  H_0 = Q - S R^-1 S'
//   Y = (I + G_k H_k)^-1 [A_k | G_k]                      (Gauss-Jordan with partial pivoting, 2n right-hand sides)
//   G_{k+1} = G_k + sym(A_k Y_2 A_k'),  H_{k+1} = H_k + sym(A_k' H_k Y_1),  A_{k+1} = A_k Y_1
// until max|H_{k+1} - H_k| <= tol max|H_{k+1}| and max|A_{k+1}| <= kSsAZero.  Then K, k, p from one pivot-free
// elimination of R + B'PB with [B'PA + S' | c_u | B'] on the right, and one pivoted solve of I - A_cl'.  The certificate
// is taken on the result: A_cl = A + BK squared until max|A_cl^(2^j)| <= kSsAZero, within max_iter squarings.
//
// Products run on v_mfma_f64_16x16x4_f64 (wave_ops_f64.h wave_matmul_f64), the pivot search on the 64-bit wave_max,
// matrix-vector terms as fma() written out.  The LDS layout is the fp32 kernels', carved from dynamic shared memory:
// 30 KiB for ss_f64_wave16 (five waves per CU), 116 KiB for ss_f64_wave32 (one; above the 64 KiB static limit, so the
// launch opts in to it).  Waves exit after their own iteration count and never talk to each other.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "launch.h"
#include "wave_ops_f64.h"

namespace tfmpc {

namespace {

using T = double;

constexpr int kSsMaxIter = 40;
constexpr double kSsTol = 4.0 * DBL_EPSILON;
constexpr double kSsAZero = 1e-3;

struct SsArgs {
    int B, n, m, max_iter;
    double tol;
    const double *F, *f, *C, *c;
    long sF, sf, sC, sc;
    double *K, *k, *P, *p;
    int32_t *iterations, *status;
};

// leading dimensions and element counts of the NP-wide LDS layout
template <int NP>
struct SsLayout {
    static constexpr int LDN = NP + 1, LDD = 2 * NP + 1, LDA = 3 * NP + 1;
    static constexpr int kF = NP * LDD, kC = 2 * NP * LDD, kSq = NP * LDN, kAug = NP * LDA;
    static constexpr int kTotal = kF + kC + NP + 2 * NP + 5 * kSq + kAug + 4 * NP;
};
static_assert(SsLayout<16>::kTotal == 3840 && SsLayout<32>::kTotal == 14848, "DESIGN.md 3.16: 30 KiB and 116 KiB");

// NP: the compile-time bound on n and m (16 or 32): the LDS tile width and the k-steps of every matrix product.
template <int NP>
__global__ __launch_bounds__(kWave) void lqr_steady_state_f64_kernel(SsArgs a)
{
    using L = SsLayout<NP>;
    constexpr int LDN = L::LDN, LDD = L::LDD, LDA = L::LDA;
    extern __shared__ double ss_smem_f64[];
    // the fp32 kernel's arrays, in its order, carved from dynamic shared memory
    T *const sF = ss_smem_f64, *const sC = sF + L::kF, *const sf = sC + L::kC, *const sc = sf + NP;
    T *const sA = sc + 2 * NP, *const sG = sA + L::kSq, *const sH = sG + L::kSq, *const sT1 = sH + L::kSq, *const sT2 = sT1 + L::kSq;
    T *const aug = sT2 + L::kSq, *const fac = aug + L::kAug, *const pf = fac + NP, *const kv = pf + NP, *const pv = kv + NP;

    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m;
    const T *Fg = a.F + (size_t)b * a.sF, *fg = a.f + (size_t)b * a.sf;
    const T *Cg = a.C + (size_t)b * a.sC, *cg = a.c + (size_t)b * a.sc;
    load_matrix(sF, LDD, Fg, n, d);
    load_matrix(sC, LDD, Cg, d, d);
    for (int i = lane; i < n; i += kWave) sf[i] = fg[i];
    for (int i = lane; i < d; i += kWave) sc[i] = cg[i];
    // element accessors of the model in LDS
    auto Am = [&](int i, int j) { return sF[i * LDD + j]; };           // A[n][n]
    auto Bm = [&](int i, int j) { return sF[i * LDD + n + j]; };       // B[n][m]
    auto zero = [](int, int) { return T(0); };
    wsync();

    int status = 0, it = 0;
    bool converged = false;

    // ---- R^-1 [S' | B'] by elimination without pivoting (a non-positive pivot <=> R not positive definite)
    wave_for_2d(m, m + 2 * n, [&](int r, int j, int) {
        T x;
        if (j < m) x = sC[(n + r) * LDD + n + j];
        else if (j < m + n) x = sC[(j - m) * LDD + n + r];             // S' = C_xu'
        else x = Bm(j - m - n, r);                                      // B'
        aug[r * LDA + j] = x;
    });
    wsync();
    if (wave_gauss_jordan<false>(aug, LDA, m, m + 2 * n, fac, fac)) status |= TFMPC_ST_NOT_PD;

    if (!status) {
        // A_0 = A - B (R^-1 S'),  G_0 = sym(B (R^-1 B')),  H_0 = sym(Q - S (R^-1 S'))
        wave_matmul_f64<NP>(n, n, m, [&](int i, int kk) { return -Bm(i, kk); }, [&](int kk, int j) { return aug[kk * LDA + m + j]; },
                            Am, [&](int i, int j, T x) { sA[i * LDN + j] = x; });
        wave_matmul_f64<NP>(n, n, m, Bm, [&](int kk, int j) { return aug[kk * LDA + m + n + j]; }, zero,
                            [&](int i, int j, T x) { sG[i * LDN + j] = x; });
        wave_matmul_f64<NP>(n, n, m, [&](int i, int kk) { return -sC[i * LDD + n + kk]; },
                            [&](int kk, int j) { return aug[kk * LDA + m + j]; }, [&](int i, int j) { return sC[i * LDD + j]; },
                            [&](int i, int j, T x) { sH[i * LDN + j] = x; });
        wsync();
        symmetrise(sG, LDN, n);
        symmetrise(sH, LDN, n);
        wsync();

        const int max_iter = a.max_iter;
        const T tol = a.tol;
        while (it < max_iter) {
            ++it;
            // aug = [I + G H | A_k | G_k]
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sG[i * LDN + kk]; }, [&](int kk, int j) { return sH[kk * LDN + j]; },
                                [](int i, int j) { return i == j ? T(1) : T(0); }, [&](int i, int j, T x) { aug[i * LDA + j] = x; });
            wave_for_2d(n, 2 * n, [&](int i, int j, int) {
                aug[i * LDA + n + j] = j < n ? sA[i * LDN + j] : sG[i * LDN + j - n];
            });
            wsync();
            if (wave_gauss_jordan<true>(aug, LDA, n, 3 * n, fac, fac)) {
                status |= TFMPC_ST_SINGULAR;
                break;
            }
            // Y_1 = aug[:, n:2n], Y_2 = aug[:, 2n:3n]; aug[:, 0:n] is free: X below
            auto Y1 = [&](int i, int j) { return aug[i * LDA + n + j]; };
            auto Y2 = [&](int i, int j) { return aug[i * LDA + 2 * n + j]; };
            auto X = [&](int i, int j) { return aug[i * LDA + j]; };
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sA[i * LDN + kk]; }, Y2, zero,
                                [&](int i, int j, T x) { sT1[i * LDN + j] = x; });           // T1 = A_k Y_2
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sH[i * LDN + kk]; }, Y1, zero,
                                [&](int i, int j, T x) { sT2[i * LDN + j] = x; });           // T2 = H_k Y_1
            wsync();
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sT1[i * LDN + kk]; }, [&](int kk, int j) { return sA[j * LDN + kk]; },
                                zero, [&](int i, int j, T x) { aug[i * LDA + j] = x; });    // X = T1 A_k'
            wsync();
            wave_for_2d(n, n, [&](int i, int j, int) { sG[i * LDN + j] += T(0.5) * (X(i, j) + X(j, i)); });
            wsync();
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sA[kk * LDN + i]; }, [&](int kk, int j) { return sT2[kk * LDN + j]; },
                                zero, [&](int i, int j, T x) { aug[i * LDA + j] = x; });    // X = A_k' T2
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sA[i * LDN + kk]; }, Y1, zero,
                                [&](int i, int j, T x) { sT1[i * LDN + j] = x; });           // T1 = A_{k+1}
            wsync();
            T dh = T(0), hmax = T(0), amax = T(0);
            bool bad = false;          // (the maximum drops a NaN operand: non-finite entries are counted on their own)
            wave_for_2d(n, n, [&](int i, int j, int) {
                const T inc = T(0.5) * (X(i, j) + X(j, i));
                const T h = sH[i * LDN + j] + inc;
                sH[i * LDN + j] = h;
                const T an = sT1[i * LDN + j];
                sA[i * LDN + j] = an;
                bad |= !(finite(h) && finite(inc) && finite(an));
                dh = fmax(dh, fabs(inc));
                hmax = fmax(hmax, fabs(h));
                amax = fmax(amax, fabs(an));
            });
            const bool nonfinite = __ballot(bad) != 0;
            dh = wave_max(dh);
            hmax = wave_max(hmax);
            amax = wave_max(amax);
            wsync();
            if (nonfinite) break;
            if (dh <= tol * hmax && amax <= kSsAZero) {
                converged = true;
                break;
            }
        }
        if (!status && !converged) status |= TFMPC_ST_NOT_STABILISING;
    }

    if (!status) {
        // P = H.  T1 = P B [n][m], T2 = P A [n][n], pf = P f
        wave_matmul_f64<NP>(n, m, n, [&](int i, int kk) { return sH[i * LDN + kk]; }, Bm, zero,
                            [&](int i, int j, T x) { sT1[i * LDN + j] = x; });
        wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sH[i * LDN + kk]; }, Am, zero,
                            [&](int i, int j, T x) { sT2[i * LDN + j] = x; });
        wave_matvec<T>(n, n, [&](int i, int j) { return sH[i * LDN + j]; }, [&](int j) { return sf[j]; }, [&](int i, T s) { pf[i] = s; });
        wsync();
        // aug = [R + B'PB | B'PA + S' | c_u | B']  (m rows)
        wave_matmul_f64<NP>(m, m, n, [&](int i, int kk) { return Bm(kk, i); }, [&](int kk, int j) { return sT1[kk * LDN + j]; },
                            [&](int i, int j) { return sC[(n + i) * LDD + n + j]; }, [&](int i, int j, T x) { aug[i * LDA + j] = x; });
        wave_matmul_f64<NP>(m, n, n, [&](int i, int kk) { return Bm(kk, i); }, [&](int kk, int j) { return sT2[kk * LDN + j]; },
                            [&](int i, int j) { return sC[j * LDD + n + i]; }, [&](int i, int j, T x) { aug[i * LDA + m + j] = x; });
        wave_for_2d(m, n + 1, [&](int r, int j, int) {
            aug[r * LDA + m + n + j] = j == 0 ? sc[n + r] : Bm(j - 1, r);
        });
        wsync();
        symmetrise(aug, LDA, m);
        wsync();
        if (wave_gauss_jordan<false>(aug, LDA, m, m + 2 * n + 1, fac, fac)) status |= TFMPC_ST_NOT_PD;
    }

    if (!status) {
        // K -> T1 [m][n], Z = (R + B'PB)^-1 B' -> G [m][n], kv = -(R + B'PB)^-1 c_u
        wave_for_2d(m, n, [&](int r, int j, int) {
            sT1[r * LDN + j] = -aug[r * LDA + m + j];
            sG[r * LDN + j] = aug[r * LDA + m + n + 1 + j];
        });
        for (int r = lane; r < m; r += kWave) kv[r] = -aug[r * LDA + m + n];
        wsync();
        // T2 = A_cl = A + B K
        wave_matmul_f64<NP>(n, n, m, Bm, [&](int kk, int j) { return sT1[kk * LDN + j]; }, Am,
                            [&](int i, int j, T x) { sT2[i * LDN + j] = x; });
        wsync();
        // aug = [I - A_cl' | c_x + K'c_u + A_cl' P f]  (n rows)
        for (int i = lane; i < n; i += kWave) {
            T s1 = T(0), s2 = T(0);
            for (int r = 0; r < m; ++r) s1 = fma(sT1[r * LDN + i], sc[n + r], s1);
            for (int j = 0; j < n; ++j) s2 = fma(sT2[j * LDN + i], pf[j], s2);
            aug[i * LDA + n] = (sc[i] + s1) + s2;
        }
        wave_for_2d(n, n, [&](int i, int j, int) { aug[i * LDA + j] = (i == j ? T(1) : T(0)) - sT2[j * LDN + i]; });
        wsync();
        if (wave_gauss_jordan<true>(aug, LDA, n, n + 1, fac, fac)) status |= TFMPC_ST_SINGULAR;
    }

    if (!status) {
        for (int i = lane; i < n; i += kWave) pv[i] = aug[i * LDA + n];
        wsync();
        // k = kv - Z (P f + p)
        wave_matvec<T>(m, n, [&](int r, int j) { return sG[r * LDN + j]; }, [&](int j) { return pf[j] + pv[j]; },
                       [&](int r, T s) { kv[r] = kv[r] - s; });
        wsync();
        bool bad = false;
        wave_for_2d(n, n, [&](int i, int j, int) { bad |= !finite(sH[i * LDN + j]); });
        wave_for_2d(m, n, [&](int i, int j, int) { bad |= !finite(sT1[i * LDN + j]); });
        for (int i = lane; i < n; i += kWave) bad |= !finite(pv[i]);
        for (int i = lane; i < m; i += kWave) bad |= !finite(kv[i]);
        if (__ballot(bad)) status |= TFMPC_ST_NOT_STABILISING;
        // Certificate on the gains themselves: A_cl^(2^j) -> 0 within max_iter squarings.  (A_k -> 0 alone does not
        // prove it: with an unstable mode that no input reaches, H_k can grow to a huge but finite value that drives
        // Y_1 = (I + G H)^-1 A_k, and so A_{k+1}, to zero.)  Squares ping-pong between T2 (A_cl) and A.
        bool certified = false;
        for (int j = 0; j < a.max_iter && !certified && !status; ++j) {
            T *src = (j & 1) ? sA : sT2, *dst = (j & 1) ? sT2 : sA;
            T mx = T(0);
            bool nf = false;
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return src[i * LDN + kk]; }, [&](int kk, int c2) { return src[kk * LDN + c2]; },
                                zero, [&](int i, int c2, T x) {
                                    dst[i * LDN + c2] = x;
                                    nf |= !finite(x);
                                    mx = fmax(mx, fabs(x));
                                });
            if (__ballot(nf)) break;
            certified = wave_max(mx) <= kSsAZero;
            wsync();
        }
        if (!certified) status |= TFMPC_ST_NOT_STABILISING;
    }

    // outputs: NaN throughout for a flagged instance
    const T qnan = __builtin_nan("");
    const bool ok = status == 0;
    if (a.K) {
        T *Ko = a.K + (size_t)b * m * n;
        wave_for_2d(m, n, [&](int i, int j, int idx) { Ko[idx] = ok ? sT1[i * LDN + j] : qnan; });
    }
    if (a.P) {
        T *Po = a.P + (size_t)b * n * n;
        wave_for_2d(n, n, [&](int i, int j, int idx) { Po[idx] = ok ? sH[i * LDN + j] : qnan; });
    }
    if (a.k)
        for (int i = lane; i < m; i += kWave) a.k[(size_t)b * m + i] = ok ? kv[i] : qnan;
    if (a.p)
        for (int i = lane; i < n; i += kWave) a.p[(size_t)b * n + i] = ok ? pv[i] : qnan;
    if (lane == 0) {
        a.status[b] = status;
        if (a.iterations) a.iterations[b] = it;
    }
}

template <int NP>
int launch_for(const SsArgs &a, hipStream_t stream)
{
    return launch_with_lds(lqr_steady_state_f64_kernel<NP>, a.B, kWave, SsLayout<NP>::kTotal * sizeof(double), stream, a);
}

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

const char *tfmpc_lqr_steady_state_kernel_name_f64(int n, int m)
{
    if (n <= 0 || m <= 0) return "invalid";
    if (wave16(n, m)) return "ss_f64_wave16";
    if (n <= 32 && m <= 32) return "ss_f64_wave32";
    return "unsupported";
}

int tfmpc_lqr_steady_state_f64(int B, int n, int m, const double *F, long sF_b, const double *f, long sf_b,
                               const double *C, long sC_b, const double *c, long sc_b, int max_iter, double tol,
                               double *K, double *k, double *P, double *p, int32_t *iterations, int32_t *status, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || max_iter < 0 || !(tol >= 0.0)) return TFMPC_ERR_ARG;
    if (n > 32 || m > 32) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;
    if (!F || !f || !C || !c || !status) return TFMPC_ERR_ARG;
    if (sF_b < 0 || sf_b < 0 || sC_b < 0 || sc_b < 0) return TFMPC_ERR_ARG;
    SsArgs a{};
    a.B = B; a.n = n; a.m = m;
    a.max_iter = max_iter ? max_iter : kSsMaxIter;
    a.tol = tol > 0.0 ? tol : kSsTol;
    a.F = F; a.f = f; a.C = C; a.c = c;
    a.sF = sF_b; a.sf = sf_b; a.sC = sC_b; a.sc = sc_b;
    a.K = K; a.k = k; a.P = P; a.p = p;
    a.iterations = iterations; a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return wave16(n, m) ? launch_for<16>(a, s) : launch_for<32>(a, s);
}

}  // extern "C"
