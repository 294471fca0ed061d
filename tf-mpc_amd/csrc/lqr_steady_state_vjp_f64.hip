// lqr_steady_state_vjp_f64.hip -- DOUBLE-PRECISION gradients of the infinite-horizon LQR (tfmpc_lqr_steady_state_vjp_f64,
// include/tfmpc_hip.h): one wavefront per instance, n <= 32 and m <= 32.
//
// The sequence of lqr_steady_state_vjp.hip, statement for statement, in double -- a change to either
// belongs in both files.  Given the forward's K, k, P, p (tfmpc_lqr_steady_state_f64) and upstream gradients gK, gk, gP, gp:
//   G = R + B'PB, A_cl = A + BK (recomputed from the saved K, P), w = Pf + p
//   [G^-1 | kappa] = G^-1 [I | gk]                       (elimination without pivoting: a non-positive pivot is NOT_PD)
//   wbar = -B kappa,  rho = (I - A_cl)^-1 (gp + wbar)    (pivoted elimination: a zero pivot is SINGULAR)
//   v = wbar + A_cl rho,  df = P v,  dc = [rho; K rho - kappa]
//   Kbar = gK + (c_u + B'w) rho',  L = -G^-1 Kbar,  Gbar = -kappa k' + L K'
//   Pbar = gP + v f' + B ([L | Gbar] F')
//   Y = A_cl Y A_cl' + sym(Pbar)                         (Smith doubling: Y += sym(Phi Y Phi'), Phi <- Phi^2, Phi_0 = A_cl)
//   dA = w rho' + [PB | P A_cl] [L; 2Y],  dB = w (K rho - kappa)' + [PA | PB | P A_cl] [L'; Gbar + Gbar'; 2 Y K']
//   dC = sym([[Y, L' + 2 Y K'], [0, Gbar + K Y K']])
// The Smith loop stops when max|Phi Y Phi'| <= tol max|Y| and max|Phi^2| <= kPhiZero, within max_iter steps; otherwise,
// or on a non-finite value, the instance is NOT_STABILISING.  A flagged instance (forward or backward) gets NaN in its
// own gradient rows.
//
// Products run on v_mfma_f64_16x16x4_f64 (wave_ops_f64.h wave_matmul_f64), the pivot search on the 64-bit wave_max,
// matrix-vector terms as fma() written out.  A product whose k-dimension is a concatenation (n + m, 2n + m) is ONE
// wave_matmul_f64 instantiated with KMAX = 2 NP or 3 NP: the k-steps past K are skipped, so the sequence of accumulations
// is the one a chain through `init` would run, without the round trip of the partial result through memory.  The LDS
// layout is the fp32 kernel's, carved from dynamic shared memory: 31.1 KiB for ss_vjp_f64_wave16 (five waves per CU),
// 118.3 KiB for ss_vjp_f64_wave32 (one; above the 64 KiB static limit, so the launch opts in to it).  A gradient whose
// batch stride is 0 is summed over the batch: the instance kernel writes per-instance records into the workspace, then
// the shared batch sum in double (batch_sum.h: chunks of 64 instances, tree over the chunks) writes the output.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/tfmpc_hip.h"
#include "batch_sum.h"
#include "launch.h"
#include "wave_ops_f64.h"

namespace tfmpc {

namespace {

using T = double;

constexpr int kVjpMaxIter = 40;
constexpr double kVjpTol = 4.0 * DBL_EPSILON;
constexpr double kPhiZero = 1e-3;
constexpr int kRedChunk = 64;          // instances per stage-1 block of the batch sum
enum { kOutF, kOutf, kOutC, kOutc, kOuts };

struct VjpOut {
    double *p;
    long sb;          // batch stride in elements (a workspace record when the caller's stride is 0)
};

struct SsVjpArgs {
    int B, n, m, max_iter;
    double tol;
    const double *F, *f, *C, *c;
    long sF, sf, sC, sc;
    const double *K, *k, *P, *p;
    const int32_t *fwd_status;
    const double *gK, *gk, *gP, *gp;
    VjpOut o[kOuts];
    int32_t *status;
};

// leading dimensions and element counts of the NP-wide LDS layout: F and aug [NP][2 NP + 1], ten square tiles, thirteen
// NP-vectors (c takes two)
template <int NP>
struct VjpLayout {
    static constexpr int LDN = NP + 1, LDD = 2 * NP + 1;
    static constexpr int kWide = NP * LDD, kSq = NP * LDN;
    static constexpr int kTotal = 2 * kWide + 10 * kSq + 13 * NP;
};
static_assert(VjpLayout<16>::kTotal == 3984 && VjpLayout<32>::kTotal == 15136, "DESIGN.md 3.22: 31.1 KiB and 118.3 KiB");

// NP: the compile-time bound on n and m (16 or 32): the LDS tile width and the k-steps of every matrix product.
template <int NP>
__global__ __launch_bounds__(kWave) void ss_vjp_f64_kernel(SsVjpArgs a)
{
    using Lay = VjpLayout<NP>;
    constexpr int LDN = Lay::LDN, LDD = Lay::LDD, SQ = Lay::kSq;
    extern __shared__ double ss_vjp_smem_f64[];
    // the fp32 kernel's arrays, in its order, carved from dynamic shared memory
    T *const sF = ss_vjp_smem_f64, *const aug = sF + Lay::kWide;
    T *const sK = aug + Lay::kWide, *const sP = sK + SQ, *const sAcl = sP + SQ, *const sPB = sAcl + SQ, *const sL = sPB + SQ;
    T *const sGb = sL + SQ, *const sY = sGb + SQ, *const sT1 = sY + SQ, *const sT2 = sT1 + SQ, *const sT3 = sT2 + SQ;
    T *const vf = sT3 + SQ, *const vc = vf + NP, *const vk = vc + 2 * NP, *const vp = vk + NP, *const vw = vp + NP;
    T *const vwbar = vw + NP, *const vrho = vwbar + NP, *const vKrho = vrho + NP, *const vv = vKrho + NP, *const vy = vv + NP;
    T *const vkap = vy + NP, *const fac = vkap + NP;

    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m;
    int status = a.fwd_status[b];
    int it = 0;
    const T *Cg = a.C + (size_t)b * a.sC;
    auto Am = [&](int i, int j) { return sF[i * LDD + j]; };           // A[n][n]
    auto Bm = [&](int i, int j) { return sF[i * LDD + n + j]; };       // B[n][m]
    auto zero = [](int, int) { return T(0); };

    if (!status) {
        load_matrix(sF, LDD, a.F + (size_t)b * a.sF, n, d);
        load_matrix(sK, LDN, a.K + (size_t)b * m * n, m, n);
        load_matrix(sP, LDN, a.P + (size_t)b * n * n, n, n);
        for (int i = lane; i < n; i += kWave) {
            vf[i] = a.f[(size_t)b * a.sf + i];
            vp[i] = a.p[(size_t)b * n + i];
        }
        for (int i = lane; i < d; i += kWave) vc[i] = a.c[(size_t)b * a.sc + i];
        for (int i = lane; i < m; i += kWave) vk[i] = a.k[(size_t)b * m + i];
        wsync();
        // PB = P B [n][m], A_cl = A + B K, w = P f + p
        wave_matmul_f64<NP>(n, m, n, [&](int i, int kk) { return sP[i * LDN + kk]; }, Bm, zero,
                            [&](int i, int j, T x) { sPB[i * LDN + j] = x; });
        wave_matmul_f64<NP>(n, n, m, Bm, [&](int kk, int j) { return sK[kk * LDN + j]; }, Am,
                            [&](int i, int j, T x) { sAcl[i * LDN + j] = x; });
        wave_matvec<T>(n, n, [&](int i, int j) { return sP[i * LDN + j]; }, [&](int j) { return vf[j]; },
                       [&](int i, T s) { vw[i] = s + vp[i]; });
        wsync();
        // aug = [R + B'PB | I | gk]  (m rows), R + B'PB symmetrised as in the forward
        wave_matmul_f64<NP>(m, m, n, [&](int i, int kk) { return Bm(kk, i); }, [&](int kk, int j) { return sPB[kk * LDN + j]; },
                            [&](int i, int j) { return Cg[(n + i) * d + n + j]; }, [&](int i, int j, T x) { aug[i * LDD + j] = x; });
        wave_for_2d(m, m + 1, [&](int r, int j, int) {
            aug[r * LDD + m + j] = j < m ? (r == j ? T(1) : T(0)) : (a.gk ? a.gk[(size_t)b * m + r] : T(0));
        });
        wsync();
        symmetrise(aug, LDD, m);
        wsync();
        if (wave_gauss_jordan<false, T>(aug, LDD, m, 2 * m + 1, fac, fac)) status |= TFMPC_ST_NOT_PD;
    }
    auto Gi = [&](int i, int j) { return aug[i * LDD + m + j]; };       // G^-1 [m][m]

    if (!status) {
        for (int r = lane; r < m; r += kWave) vkap[r] = aug[r * LDD + 2 * m];
        wsync();
        // wbar = -B kappa;  T1 = [I - A_cl | gp + wbar]  (n rows)
        wave_matvec<T>(n, m, Bm, [&](int r) { return vkap[r]; }, [&](int i, T s) {
            vwbar[i] = -s;
            sT1[i * LDN + n] = (a.gp ? a.gp[(size_t)b * n + i] : T(0)) - s;
        });
        wave_for_2d(n, n, [&](int i, int j, int) { sT1[i * LDN + j] = (i == j ? T(1) : T(0)) - sAcl[i * LDN + j]; });
        wsync();
        if (wave_gauss_jordan<true, T>(sT1, LDN, n, n + 1, fac, fac)) status |= TFMPC_ST_SINGULAR;
    }

    if (!status) {
        for (int i = lane; i < n; i += kWave) vrho[i] = sT1[i * LDN + n];
        wsync();
        // K rho, v = wbar + A_cl rho, y = c_u + B'w
        for (int r = lane; r < m; r += kWave) {
            T s1 = T(0), s2 = T(0);
            for (int j = 0; j < n; ++j) {
                s1 = fma(sK[r * LDN + j], vrho[j], s1);
                s2 = fma(Bm(j, r), vw[j], s2);
            }
            vKrho[r] = s1;
            vy[r] = vc[n + r] + s2;
        }
        wave_matvec<T>(n, n, [&](int i, int j) { return sAcl[i * LDN + j]; }, [&](int j) { return vrho[j]; },
                       [&](int i, T s) { vv[i] = vwbar[i] + s; });
        wsync();
        // T2 = Kbar = gK + y rho'  [m][n]
        wave_for_2d(m, n, [&](int i, int j, int idx) {
            sT2[i * LDN + j] = fma(vy[i], vrho[j], a.gK ? a.gK[(size_t)b * m * n + idx] : T(0));
        });
        wsync();
        // L = -G^-1 Kbar [m][n]
        wave_matmul_f64<NP>(m, n, m, [&](int i, int kk) { return -Gi(i, kk); }, [&](int kk, int j) { return sT2[kk * LDN + j]; }, zero,
                            [&](int i, int j, T x) { sL[i * LDN + j] = x; });
        wsync();
        // Gbar = -kappa k' + L K' [m][m]
        wave_matmul_f64<NP>(m, m, n, [&](int i, int kk) { return sL[i * LDN + kk]; }, [&](int kk, int j) { return sK[j * LDN + kk]; },
                            [&](int i, int j) { return -(vkap[i] * vk[j]); }, [&](int i, int j, T x) { sGb[i * LDN + j] = x; });
        wsync();
        // T2 = U = [L | Gbar] F'  [m][n]
        wave_matmul_f64<2 * NP>(m, n, d, [&](int i, int kk) { return kk < n ? sL[i * LDN + kk] : sGb[i * LDN + kk - n]; },
                                [&](int kk, int j) { return sF[j * LDD + kk]; }, zero, [&](int i, int j, T x) { sT2[i * LDN + j] = x; });
        wsync();
        // T1 = Pbar = gP + v f' + B U  [n][n]
        wave_matmul_f64<NP>(n, n, m, Bm, [&](int kk, int j) { return sT2[kk * LDN + j]; },
                            [&](int i, int j) { return fma(vv[i], vf[j], a.gP ? a.gP[(size_t)b * n * n + i * n + j] : T(0)); },
                            [&](int i, int j, T x) { sT1[i * LDN + j] = x; });
        wsync();
        wave_for_2d(n, n, [&](int i, int j, int) { sY[i * LDN + j] = T(0.5) * (sT1[i * LDN + j] + sT1[j * LDN + i]); });
        wsync();

        // Smith doubling on Y = A_cl Y A_cl' + sym(Pbar): Phi ping-pongs between A_cl's tile and T3
        T *phi = sAcl, *phi2 = sT3;
        bool converged = false;
        while (it < a.max_iter) {
            ++it;
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return phi[i * LDN + kk]; }, [&](int kk, int j) { return sY[kk * LDN + j]; },
                                zero, [&](int i, int j, T x) { sT2[i * LDN + j] = x; });          // T2 = Phi Y
            wsync();
            T pmax = T(0);
            bool bad = false;          // (fmax drops a NaN operand: non-finite entries are counted on their own)
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sT2[i * LDN + kk]; }, [&](int kk, int j) { return phi[j * LDN + kk]; },
                                zero, [&](int i, int j, T x) { sT1[i * LDN + j] = x; });          // T1 = Phi Y Phi'
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return phi[i * LDN + kk]; }, [&](int kk, int j) { return phi[kk * LDN + j]; },
                                zero, [&](int i, int j, T x) {
                                    phi2[i * LDN + j] = x;
                                    bad |= !finite(x);
                                    pmax = fmax(pmax, fabs(x));
                                });                                                                // Phi^2
            wsync();
            T dmax = T(0), ymax = T(0);
            wave_for_2d(n, n, [&](int i, int j, int) {
                const T x = sT1[i * LDN + j];
                const T y = sY[i * LDN + j] + T(0.5) * (x + sT1[j * LDN + i]);
                sY[i * LDN + j] = y;
                bad |= !(finite(x) && finite(y));
                dmax = fmax(dmax, fabs(x));
                ymax = fmax(ymax, fabs(y));
            });
            const bool nonfinite = __ballot(bad) != 0;
            dmax = wave_max(dmax);
            ymax = wave_max(ymax);
            pmax = wave_max(pmax);
            T *t = phi;
            phi = phi2;
            phi2 = t;
            wsync();
            if (nonfinite) break;
            if (dmax <= a.tol * ymax && pmax <= kPhiZero) {
                converged = true;
                break;
            }
        }
        if (!converged) status |= TFMPC_ST_NOT_STABILISING;
    }

    const bool ok = status == 0;
    if (ok) {
        // T1 = K Y [m][n], T2 = P A [n][n]; then Acl's tile = W = P A_cl = PA + PB K, T3 = Rbar = Gbar + (KY) K' [m][m]
        wave_matmul_f64<NP>(m, n, n, [&](int i, int kk) { return sK[i * LDN + kk]; }, [&](int kk, int j) { return sY[kk * LDN + j]; }, zero,
                            [&](int i, int j, T x) { sT1[i * LDN + j] = x; });
        wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sP[i * LDN + kk]; }, Am, zero,
                            [&](int i, int j, T x) { sT2[i * LDN + j] = x; });
        wsync();
        wave_matmul_f64<NP>(n, n, m, [&](int i, int kk) { return sPB[i * LDN + kk]; }, [&](int kk, int j) { return sK[kk * LDN + j]; },
                            [&](int i, int j) { return sT2[i * LDN + j]; }, [&](int i, int j, T x) { sAcl[i * LDN + j] = x; });
        wave_matmul_f64<NP>(m, m, n, [&](int i, int kk) { return sT1[i * LDN + kk]; }, [&](int kk, int j) { return sK[j * LDN + kk]; },
                            [&](int i, int j) { return sGb[i * LDN + j]; }, [&](int i, int j, T x) { sT3[i * LDN + j] = x; });
        wsync();
        const VjpOut &oF = a.o[kOutF], &of = a.o[kOutf], &oC = a.o[kOutC], &oc = a.o[kOutc];
        if (oF.p) {
            T *dF = oF.p + (size_t)b * oF.sb;
            // dA = w rho' + [PB | W] [L; 2Y]
            wave_matmul_f64<2 * NP>(n, n, m + n, [&](int i, int kk) { return kk < m ? sPB[i * LDN + kk] : sAcl[i * LDN + kk - m]; },
                                    [&](int kk, int j) { return kk < m ? sL[kk * LDN + j] : T(2) * sY[(kk - m) * LDN + j]; },
                                    [&](int i, int j) { return vw[i] * vrho[j]; }, [&](int i, int j, T x) { dF[i * d + j] = x; });
            // dB = w (K rho - kappa)' + [PA | PB | W] [L'; Gbar + Gbar'; 2 (KY)']
            wave_matmul_f64<3 * NP>(n, m, 2 * n + m,
                                    [&](int i, int kk) {
                                        return kk < n ? sT2[i * LDN + kk] : kk < n + m ? sPB[i * LDN + kk - n] : sAcl[i * LDN + kk - n - m];
                                    },
                                    [&](int kk, int j) {
                                        return kk < n ? sL[j * LDN + kk]
                                               : kk < n + m ? sGb[(kk - n) * LDN + j] + sGb[j * LDN + kk - n]
                                                            : T(2) * sT1[j * LDN + kk - n - m];
                                    },
                                    [&](int i, int j) { return vw[i] * (vKrho[j] - vkap[j]); },
                                    [&](int i, int j, T x) { dF[i * d + n + j] = x; });
        }
        if (oC.p) {
            T *dC = oC.p + (size_t)b * oC.sb;
            auto Sbar = [&](int i, int j) { return sL[j * LDN + i] + T(2) * sT1[j * LDN + i]; };      // L' + 2 (KY)' [n][m]
            wave_for_2d(d, d, [&](int i, int j, int idx) {
                T x;
                if (i < n && j < n) x = T(0.5) * (sY[i * LDN + j] + sY[j * LDN + i]);
                else if (i < n) x = T(0.5) * Sbar(i, j - n);
                else if (j < n) x = T(0.5) * Sbar(j, i - n);
                else x = T(0.5) * (sT3[(i - n) * LDN + j - n] + sT3[(j - n) * LDN + i - n]);
                dC[idx] = x;
            });
        }
        if (of.p) {
            T *df = of.p + (size_t)b * of.sb;
            wave_matvec<T>(n, n, [&](int i, int j) { return sP[i * LDN + j]; }, [&](int j) { return vv[j]; }, [&](int i, T s) { df[i] = s; });
        }
        if (oc.p) {
            T *dc = oc.p + (size_t)b * oc.sb;
            for (int i = lane; i < d; i += kWave) dc[i] = i < n ? vrho[i] : vKrho[i - n] - vkap[i - n];
        }
    } else {
        const int sizes[kOuts] = {n * d, n, d * d, d};
        for (int k = 0; k < kOuts; ++k)
            if (a.o[k].p) fill_nan(a.o[k].p + (size_t)b * a.o[k].sb, sizes[k]);
    }
    if (lane == 0) a.status[b] = status;
}

// the batch sum's workspace layout for the summed ones of dF, df, dC, dc (element counts: doubles here)
BatchSumPlan sum_plan(int B, int n, int m, unsigned summed)
{
    const int d = n + m;
    const int sizes[kOuts] = {n * d, n, d * d, d}, slots[kOuts] = {1, 1, 1, 1};
    return batch_sum_plan(B, kRedChunk, kOuts, sizes, slots, summed);
}

template <int NP>
int launch_for(const SsVjpArgs &a, hipStream_t stream)
{
    return launch_with_lds(ss_vjp_f64_kernel<NP>, a.B, kWave, VjpLayout<NP>::kTotal * sizeof(double), stream, a);
}

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

size_t tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(int B, int n, int m)
{
    if (B <= 1 || n <= 0 || m <= 0 || n > 32 || m > 32) return 0;
    return sum_plan(B, n, m, (1u << kOuts) - 1).floats * sizeof(double);
}

const char *tfmpc_lqr_steady_state_vjp_kernel_name_f64(int n, int m)
{
    if (n <= 0 || m <= 0) return "invalid";
    if (wave16(n, m)) return "ss_vjp_f64_wave16";
    if (n <= 32 && m <= 32) return "ss_vjp_f64_wave32";
    return "unsupported";
}

int tfmpc_lqr_steady_state_vjp_f64(int B, int n, int m,
                                   const double *F, long sF_b, const double *f, long sf_b, const double *C, long sC_b,
                                   const double *c, long sc_b,
                                   const double *K, const double *k, const double *P, const double *p, const int32_t *fwd_status,
                                   const double *gK, const double *gk, const double *gP, const double *gp,
                                   int max_iter, double tol,
                                   double *dF, long sdF_b, double *df, long sdf_b, double *dC, long sdC_b, double *dc, long sdc_b,
                                   int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || max_iter < 0 || !(tol >= 0.0)) return TFMPC_ERR_ARG;
    if (n > 32 || m > 32) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;
    if (!F || !f || !C || !c || !K || !k || !P || !p || !fwd_status || !status) return TFMPC_ERR_ARG;
    for (long s : {sF_b, sf_b, sC_b, sc_b, sdF_b, sdf_b, sdC_b, sdc_b})
        if (s < 0) return TFMPC_ERR_ARG;
    double *outs[kOuts] = {dF, df, dC, dc};
    const long strides[kOuts] = {sdF_b, sdf_b, sdC_b, sdc_b};
    // a stride of 0 sums over the batch (no time axis here)
    const unsigned summed = batch_sum_select(B, kOuts, outs, strides, nullptr, 1, nullptr);
    const BatchSumPlan plan = sum_plan(B, n, m, summed);
    if (!plan.fits) return TFMPC_ERR_UNSUPPORTED;
    if (plan.floats && (!workspace || workspace_bytes < plan.floats * sizeof(double))) return TFMPC_ERR_WORKSPACE;
    double *w = static_cast<double *>(workspace);

    SsVjpArgs a{};
    a.B = B; a.n = n; a.m = m;
    a.max_iter = max_iter ? max_iter : kVjpMaxIter;
    a.tol = tol > 0.0 ? tol : kVjpTol;
    a.F = F; a.f = f; a.C = C; a.c = c;
    a.sF = sF_b; a.sf = sf_b; a.sC = sC_b; a.sc = sc_b;
    a.K = K; a.k = k; a.P = P; a.p = p; a.fwd_status = fwd_status;
    a.gK = gK; a.gk = gk; a.gP = gP; a.gp = gp;
    batch_sum_route(plan, w, outs, strides, nullptr, [&](int q, double *p, long b, long) { a.o[q] = {p, b}; });
    a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = wave16(n, m) ? launch_for<16>(a, s) : launch_for<32>(a, s);
    if (rc != TFMPC_OK) return rc;
    return batch_sum_run<kRedChunk, kSumTree, double>(plan, w, outs, strides, s);
}

}  // extern "C"
