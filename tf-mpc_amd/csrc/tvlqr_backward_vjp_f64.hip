// tvlqr_backward_vjp_f64.hip -- DOUBLE-PRECISION gradients of the finite-horizon Riccati recursion
// (tfmpc_tvlqr_backward_vjp_f64, include/tfmpc_hip.h): one wavefront per instance, n <= 32 and m <= 32.
//
// The sequence of tvlqr_backward_vjp.hip, statement for statement, in double -- a change to either
// belongs in both files.  Given the recursion's K_t, k_t, V_t, v_t (tfmpc_tvlqr_backward_f64) and upstream gradients gK,
// gk, gV, gv, gconst, the wave sweeps FORWARD in time carrying the adjoints Vbar (n x n, symmetric), vbar (n) and abar
// (scalar) of V_t, v_t and const_t.  With P = V_{t+1}, s = v_{t+1} (the final cost at t = T-1), step t is
//   Vbar += sym(gV_t), vbar += gv_t, abar += gconst_t
//   Quu = C_t,uu + F_t,u' P F_t,u;  [Kt | kt] = -Quu^-1 [gK_t | gk_t]   (elimination without pivoting: NOT_PD on a pivot <= 0)
//   qbar = [vbar; kt + K vbar + abar k]
//   Qbar_xx = Vbar,  Qbar_ux = (KV + G + k vbar') / 2,  Qbar_uu = sym(G K' + (qbar_u - abar k / 2) k'),  KV = K Vbar, G = KV + Kt
//   dC_t = Qbar, dc_t = qbar;  r = P f_t + s, rbar = F_t qbar;  dF_t = 2 (P F_t) Qbar + r qbar',  df_t = P rbar + abar r
//   Vbar <- sym(F_t Qbar F_t' + rbar f_t' + abar f_t f_t' / 2),  vbar <- rbar + abar f_t
// and after the last step Vbar, vbar are the final cost's gradient (added into dC_{T-1}[:n,:n], dc_{T-1}[:n] for the default
// final cost).  The propagation Vbar <- F Qbar F' is the closed loop A_cl Vbar A_cl': error does not compound with the
// horizon, which is why the fp32 sequence can be kept (unlike the costate recursion of DESIGN.md 3.15).
//
// Products run on v_mfma_f64_16x16x4_f64 (wave_ops_f64.h wave_matmul_f64<KMAX>, KMAX = NP or, where k = d, 2 NP),
// matrix-vector terms as fma() written out, the elimination and the rest on wave_ops.h's templates instantiated with
// double.  The LDS layout is the fp32 kernel's with m <= NP, carved from dynamic shared memory: 36.75 KiB for
// tvb_vjp_f64_wave16 (four waves per CU), 141.5 KiB for tvb_vjp_f64_wave32 (one; above the 64 KiB static limit, so the
// launch opts in to it).  A gradient whose time stride is 0 is accumulated in the output in time order (a lane owns the
// same elements at every step); one whose batch stride is 0 is written as per-instance records into the workspace and
// summed by the shared batch sum in double (batch_sum.h: chunks of 64 instances, tree over the chunks).  A flagged
// instance (forward or here) gets NaN in its own rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/tfmpc_hip.h"
#include "batch_sum.h"
#include "launch.h"
#include "tvlqr_kernels.h"
#include "wave_ops_f64.h"

namespace tfmpc {

namespace {

using T = double;

constexpr int kRedChunk = 64;          // instances per stage-1 block of the batch sum
enum { kOutF, kOutf, kOutC, kOutc, kOutCf, kOutcf, kOuts };

struct BvOut {
    double *p;
    long sb, st;      // batch / time stride in elements (a workspace record when the caller's batch stride is 0)
};

struct BvArgs {
    int B, n, m, T;
    const double *F, *f, *C, *c;
    long sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t;
    const double *Cfin, *cfin;         // both NULL: the default final cost
    long sCfin_b, scfin_b;
    const double *K, *k, *V, *v;
    const int32_t *fwd_status;
    const double *gK, *gk, *gV, *gv, *gconst;
    BvOut o[kOuts];
    int32_t *status;
};

__device__ __forceinline__ void emit(const BvOut &o, int b, int t, int e, double x)
{
    double *p = o.p + (size_t)b * o.sb + (size_t)t * o.st + e;
    if (o.st == 0 && t > 0) x += *p;   // time-shared: accumulate in time order (this lane owns element e at every step)
    *p = x;
}

// leading dimensions and element counts of the NP-wide LDS layout (the fp32 kernel's arrays with m <= NP): F, PF, T
// [NP][2 NP + 1] and Qbar [2 NP][2 NP + 1]; P, Vbar, K, KV, G [NP][NP + 1]; aug [NP][2 NP + 3]; nine NP-vectors (qbar
// takes two)
template <int NP>
struct BvLayout {
    static constexpr int DP = 2 * NP, LDN = NP + 1, LDD = DP + 1, LDA = 2 * NP + 3;
    static constexpr int kWide = NP * LDD, kSq = NP * LDN, kAug = NP * LDA;
    static constexpr int kTotal = 5 * kWide + 5 * kSq + kAug + 9 * NP;
};
static_assert(BvLayout<16>::kTotal == 4704 && BvLayout<32>::kTotal == 18112, "DESIGN.md 3.23: 36.75 KiB and 141.5 KiB");

// NP: the compile-time bound on n and m (16 or 32): the LDS tile width and the k-steps of every matrix product.
template <int NP>
__global__ __launch_bounds__(kWave) void tvb_vjp_f64_kernel(BvArgs a)
{
    using Lay = BvLayout<NP>;
    constexpr int LDN = Lay::LDN, LDD = Lay::LDD, LDA = Lay::LDA, WD = Lay::kWide, SQ = Lay::kSq;
    extern __shared__ double tvb_vjp_smem_f64[];
    // the fp32 kernel's arrays, in its order, carved from dynamic shared memory
    T *const sF = tvb_vjp_smem_f64, *const sPF = sF + WD, *const sT = sPF + WD, *const sQb = sT + WD;
    T *const sP = sQb + 2 * WD, *const sVb = sP + SQ, *const sK = sVb + SQ, *const sKV = sK + SQ, *const sG = sKV + SQ;
    T *const aug = sG + SQ;
    T *const vf = aug + Lay::kAug, *const vs = vf + NP, *const vk = vs + NP, *const vvb = vk + NP, *const vr = vvb + NP;
    T *const vrb = vr + NP, *const vq = vrb + NP, *const fac = vq + 2 * NP;

    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, TT = a.T, d = n + m;
    const bool dflt = a.Cfin == nullptr;
    int status = a.fwd_status[b];
    T abar = T(0);
    auto zero = [](int, int) { return T(0); };
    const BvOut &oF = a.o[kOutF], &of = a.o[kOutf], &oC = a.o[kOutC], &oc = a.o[kOutc];

    wave_for_2d(n, n, [&](int i, int j, int) { sVb[i * LDN + j] = T(0); });
    for (int i = lane; i < n; i += kWave) vvb[i] = T(0);

    for (int t = 0; t < TT && !status; ++t) {
        const size_t bt = (size_t)b * TT + t;
        const bool last = t == TT - 1;
        const T *Ft = tv_at(a.F, a.sF_b, a.sF_t, b, t), *ft = tv_at(a.f, a.sf_b, a.sf_t, b, t);
        const T *Cg = tv_at(a.C, a.sC_b, a.sC_t, b, t);
        // P = V_{t+1}, s = v_{t+1}; at the last step the final cost (default: C_{T-1}[:n,:n] with row stride d, c_{T-1}[:n])
        const T *Pg, *sg;
        int ldP = n;
        if (!last) {
            Pg = a.V + (bt + 1) * n * n;
            sg = a.v + (bt + 1) * n;
        } else if (dflt) {
            Pg = Cg;
            ldP = d;
            sg = tv_at(a.c, a.sc_b, a.sc_t, b, t);
        } else {
            Pg = a.Cfin + (size_t)b * a.sCfin_b;
            sg = a.cfin + (size_t)b * a.scfin_b;
        }
        load_matrix(sF, LDD, Ft, n, d);
        load_matrix(sK, LDN, a.K + bt * m * n, m, n);
        wave_for_2d(n, n, [&](int i, int j, int idx) {
            sP[i * LDN + j] = Pg[i * ldP + j];
            if (a.gV) sVb[i * LDN + j] += T(0.5) * (a.gV[bt * n * n + idx] + a.gV[bt * n * n + j * n + i]);
        });
        for (int i = lane; i < n; i += kWave) {
            vf[i] = ft[i];
            vs[i] = sg[i];
            if (a.gv) vvb[i] += a.gv[bt * n + i];
        }
        for (int r = lane; r < m; r += kWave) vk[r] = a.k[bt * m + r];
        // aug = [Quu | gK_t | gk_t]  (m rows)
        wave_for_2d(m, n + 1, [&](int r, int j, int) {
            aug[r * LDA + m + j] = j < n ? (a.gK ? a.gK[bt * m * n + r * n + j] : T(0)) : (a.gk ? a.gk[bt * m + r] : T(0));
        });
        if (a.gconst) abar += a.gconst[bt];
        wsync();

        // PF = P F [n][d], KV = K Vbar [m][n], r = P f + s
        wave_matmul_f64<NP>(n, d, n, [&](int i, int kk) { return sP[i * LDN + kk]; }, [&](int kk, int j) { return sF[kk * LDD + j]; },
                            zero, [&](int i, int j, T x) { sPF[i * LDD + j] = x; });
        wave_matmul_f64<NP>(m, n, n, [&](int i, int kk) { return sK[i * LDN + kk]; }, [&](int kk, int j) { return sVb[kk * LDN + j]; },
                            zero, [&](int i, int j, T x) { sKV[i * LDN + j] = x; });
        wave_matvec<T>(n, n, [&](int i, int j) { return sP[i * LDN + j]; }, [&](int j) { return vf[j]; },
                       [&](int i, T s) { vr[i] = s + vs[i]; });
        lds_sync();
        // Quu = C_uu + F_u' (P F)_u, symmetrised as in the forward
        wave_matmul_f64<NP>(m, m, n, [&](int i, int kk) { return sF[kk * LDD + n + i]; }, [&](int kk, int j) { return sPF[kk * LDD + n + j]; },
                            [&](int i, int j) { return Cg[(n + i) * d + n + j]; }, [&](int i, int j, T x) { aug[i * LDA + j] = x; });
        wsync();
        symmetrise(aug, LDA, m);
        wsync();
        if (wave_gauss_jordan<false, T>(aug, LDA, m, m + n + 1, fac, fac)) {
            status |= TFMPC_ST_NOT_PD;
            break;
        }
        // G = KV + Kt [m][n];  qbar = [vbar; kt + K vbar + abar k]
        wave_for_2d(m, n, [&](int r, int j, int) { sG[r * LDN + j] = sKV[r * LDN + j] - aug[r * LDA + m + j]; });
        for (int i = lane; i < n; i += kWave) vq[i] = vvb[i];
        wave_matvec<T>(m, n, [&](int r, int j) { return sK[r * LDN + j]; }, [&](int j) { return vvb[j]; },
                       [&](int r, T s) { vq[n + r] = fma(abar, vk[r], s - aug[r * LDA + m + n]); });
        lds_sync();
        // Qbar: the uu block (symmetrised below), xx = Vbar, ux / xu;  rbar = F qbar
        wave_matmul_f64<NP>(m, m, n, [&](int i, int kk) { return sG[i * LDN + kk]; }, [&](int kk, int j) { return sK[j * LDN + kk]; },
                            [&](int i, int j) { return (vq[n + i] - T(0.5) * abar * vk[i]) * vk[j]; },
                            [&](int i, int j, T x) { sQb[(n + i) * LDD + n + j] = x; });
        wave_for_2d(n, n, [&](int i, int j, int) { sQb[i * LDD + j] = sVb[i * LDN + j]; });
        wave_for_2d(m, n, [&](int r, int i, int) {
            const T x = T(0.5) * (sKV[r * LDN + i] + sG[r * LDN + i] + vk[r] * vvb[i]);
            sQb[(n + r) * LDD + i] = x;
            sQb[i * LDD + n + r] = x;
        });
        wave_matvec<T>(n, d, [&](int i, int j) { return sF[i * LDD + j]; }, [&](int j) { return vq[j]; }, [&](int i, T s) { vrb[i] = s; });
        lds_sync();
        symmetrise(sQb + n * LDD + n, LDD, m);
        lds_sync();
        // dF = 2 (PF) Qbar + r qbar';  T = F Qbar [n][d];  df = P rbar + abar r
        if (oF.p)
            wave_matmul_f64<2 * NP>(n, d, d, [&](int i, int kk) { return sPF[i * LDD + kk]; },
                                    [&](int kk, int j) { return T(2) * sQb[kk * LDD + j]; }, [&](int i, int j) { return vr[i] * vq[j]; },
                                    [&](int i, int j, T x) { emit(oF, b, t, i * d + j, x); });
        wave_matmul_f64<2 * NP>(n, d, d, [&](int i, int kk) { return sF[i * LDD + kk]; }, [&](int kk, int j) { return sQb[kk * LDD + j]; },
                                zero, [&](int i, int j, T x) { sT[i * LDD + j] = x; });
        if (of.p)
            wave_matvec<T>(n, n, [&](int i, int j) { return sP[i * LDN + j]; }, [&](int j) { return vrb[j]; },
                           [&](int i, T s) { emit(of, b, t, i, fma(abar, vr[i], s)); });
        lds_sync();
        // Vbar <- sym(T F' + rbar f' + abar f f' / 2) (through PF's tile), vbar <- rbar + abar f
        wave_matmul_f64<2 * NP>(n, n, d, [&](int i, int kk) { return sT[i * LDD + kk]; }, [&](int kk, int j) { return sF[j * LDD + kk]; },
                                [&](int i, int j) { return (vrb[i] + T(0.5) * abar * vf[i]) * vf[j]; },
                                [&](int i, int j, T x) { sPF[i * LDD + j] = x; });
        lds_sync();
        wave_for_2d(n, n, [&](int i, int j, int) { sVb[i * LDN + j] = T(0.5) * (sPF[i * LDD + j] + sPF[j * LDD + i]); });
        for (int i = lane; i < n; i += kWave) vvb[i] = fma(abar, vf[i], vrb[i]);
        lds_sync();
        // dC = Qbar, dc = qbar; the default final cost's gradient joins the last step's
        const bool fin = last && dflt;
        if (oC.p)
            wave_for_2d(d, d, [&](int i, int j, int idx) {
                T x = sQb[i * LDD + j];
                if (fin && i < n && j < n) x += sVb[i * LDN + j];
                emit(oC, b, t, idx, x);
            });
        if (oc.p)
            for (int i = lane; i < d; i += kWave) emit(oc, b, t, i, (fin && i < n) ? vq[i] + vvb[i] : vq[i]);
        lds_sync();
    }

    const int sizes[kOuts] = {n * d, n, d * d, d, n * n, n};
    if (!status) {
        const BvOut &oCf = a.o[kOutCf], &ocf = a.o[kOutcf];
        if (oCf.p) wave_for_2d(n, n, [&](int i, int j, int idx) { oCf.p[(size_t)b * oCf.sb + idx] = sVb[i * LDN + j]; });
        if (ocf.p)
            for (int i = lane; i < n; i += kWave) ocf.p[(size_t)b * ocf.sb + i] = vvb[i];
    } else {
        for (int q = 0; q < kOuts; ++q) {
            const BvOut &o = a.o[q];
            if (!o.p) continue;
            const int slots = (q < kOutCf && o.st) ? TT : 1;
            for (int t = 0; t < slots; ++t) fill_nan(o.p + (size_t)b * o.sb + (size_t)t * o.st, sizes[q]);
        }
    }
    if (lane == 0) a.status[b] = status;
}

bool shape_supported(int n, int m) { return n <= 32 && m <= 32; }

// the batch sum's workspace layout for the summed ones of dF, df, dC, dc (slots[q] = T or 1) and dCfin, dcfin (element
// counts: doubles here)
BatchSumPlan sum_plan(int B, int n, int m, const int slots[kOuts], unsigned summed)
{
    const int d = n + m;
    const int sizes[kOuts] = {n * d, n, d * d, d, n * n, n};
    return batch_sum_plan(B, kRedChunk, kOuts, sizes, slots, summed);
}

template <int NP>
int launch_for(const BvArgs &a, hipStream_t stream)
{
    return launch_with_lds(tvb_vjp_f64_kernel<NP>, a.B, kWave, BvLayout<NP>::kTotal * sizeof(double), stream, a);
}

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

size_t tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(int B, int n, int m, int T)
{
    if (B <= 1 || n <= 0 || m <= 0 || T <= 0 || !shape_supported(n, m)) return 0;
    const int slots[kOuts] = {T, T, T, T, 1, 1};
    return sum_plan(B, n, m, slots, (1u << kOuts) - 1).floats * sizeof(double);
}

const char *tfmpc_tvlqr_backward_vjp_kernel_name_f64(int n, int m, int T)
{
    if (n <= 0 || m <= 0 || T <= 0) return "invalid";
    if (wave16(n, m)) return "tvb_vjp_f64_wave16";
    if (shape_supported(n, m)) return "tvb_vjp_f64_wave32";
    return "unsupported";
}

int tfmpc_tvlqr_backward_vjp_f64(int B, int n, int m, int T,
                                 const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                                 const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                                 const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                                 const double *K, const double *k, const double *V, const double *v, const int32_t *fwd_status,
                                 const double *gK, const double *gk, const double *gV, const double *gv, const double *gconst,
                                 double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                                 double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t,
                                 double *dCfin, long sdCfin_b, double *dcfin, long sdcfin_b,
                                 int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!shape_supported(n, m)) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;
    if (!F || !f || !C || !c || !K || !k || !V || !v || !fwd_status || !status) return TFMPC_ERR_ARG;
    if (!Cfin != !cfin) return TFMPC_ERR_ARG;
    if (!Cfin && (dCfin || dcfin)) return TFMPC_ERR_ARG;           // the default final cost's gradient is in dC, dc
    for (long s : {sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t, sCfin_b, scfin_b, sdF_b, sdF_t, sdf_b, sdf_t, sdC_b, sdC_t,
                   sdc_b, sdc_t, sdCfin_b, sdcfin_b})
        if (s < 0) return TFMPC_ERR_ARG;
    double *outs[kOuts] = {dF, df, dC, dc, dCfin, dcfin};
    const long sb[kOuts] = {sdF_b, sdf_b, sdC_b, sdc_b, sdCfin_b, sdcfin_b};
    const long st[kOuts] = {sdF_t, sdf_t, sdC_t, sdc_t, 0, 0};
    // a batch stride of 0 sums over the batch; over a batch of one the sum is the instance's own gradient, written in place
    unsigned summed = 0;
    int slots[kOuts];
    for (int q = 0; q < kOuts; ++q) {
        slots[q] = st[q] ? T : 1;
        if (outs[q] && sb[q] == 0 && B > 1) summed |= 1u << q;
    }
    const BatchSumPlan plan = sum_plan(B, n, m, slots, summed);
    if (!plan.fits) return TFMPC_ERR_UNSUPPORTED;                  // the batch sum's blocks are one grid axis
    if (plan.floats && (!workspace || workspace_bytes < plan.floats * sizeof(double))) return TFMPC_ERR_WORKSPACE;
    double *w = static_cast<double *>(workspace);

    BvArgs a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = F; a.f = f; a.C = C; a.c = c;
    a.sF_b = sF_b; a.sF_t = sF_t; a.sf_b = sf_b; a.sf_t = sf_t; a.sC_b = sC_b; a.sC_t = sC_t; a.sc_b = sc_b; a.sc_t = sc_t;
    a.Cfin = Cfin; a.cfin = cfin; a.sCfin_b = sCfin_b; a.scfin_b = scfin_b;
    a.K = K; a.k = k; a.V = V; a.v = v; a.fwd_status = fwd_status;
    a.gK = gK; a.gk = gk; a.gV = gV; a.gv = gv; a.gconst = gconst;
    for (int q = 0; q < kOuts; ++q) {
        const long size = plan.size[q];
        if (summed >> q & 1u) a.o[q] = {w + plan.rec_off[q], (long)slots[q] * size, st[q] ? size : 0};
        else a.o[q] = {outs[q], sb[q], st[q]};
    }
    a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = wave16(n, m) ? launch_for<16>(a, s) : launch_for<32>(a, s);
    if (rc != TFMPC_OK) return rc;
    return batch_sum_run<kRedChunk, kSumTree, double>(plan, w, outs, st, s);
}

}  // extern "C"
