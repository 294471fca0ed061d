// tvlqr_backward_vjp.hip -- gradients of the finite-horizon Riccati recursion (tfmpc_tvlqr_backward_vjp_f32,
// include/tfmpc_hip.h).
//
// Given the recursion's K_t, k_t, V_t, v_t (tfmpc_tvlqr_backward_f32) and upstream gradients gK, gk, gV, gv, gconst, one
// wavefront per instance sweeps FORWARD in time carrying the adjoints Vbar (n x n, symmetric), vbar (n) and abar (scalar)
// of V_t, v_t and const_t.  With P = V_{t+1}, s = v_{t+1} (the final cost at t = T-1), L = [I; K_t], l = [0; k_t], step t is
//   Vbar += sym(gV_t), vbar += gv_t, abar += gconst_t
//   Quu = C_t,uu + F_t,u' P F_t,u;  [Kt | kt] = -Quu^-1 [gK_t | gk_t]   (elimination without pivoting: NOT_PD on a pivot <= 0)
//   qbar = [vbar; kt + K vbar + abar k]
//   Qbar = sym(L Vbar L' + E Kt L' + (w + abar l / 2) l'),  w = qbar - abar l, written by blocks with KV = K Vbar, G = KV + Kt:
//          Qbar_xx = Vbar,  Qbar_ux = (KV + G + k vbar') / 2,  Qbar_uu = sym(G K' + (qbar_u - abar k / 2) k')
//   dC_t = Qbar, dc_t = qbar;  r = P f_t + s, rbar = F_t qbar;  dF_t = 2 (P F_t) Qbar + r qbar',  df_t = P rbar + abar r
//   Vbar <- sym(F_t Qbar F_t' + rbar f_t' + abar f_t f_t' / 2),  vbar <- rbar + abar f_t
// and after the last step Vbar, vbar are the final cost's gradient (added into dC_{T-1}[:n,:n], dc_{T-1}[:n] for the default
// final cost).  The Riccati recursion is not recomputed: the sweep reads the model and the forward's outputs only.
// tvlqr_backward_vjp_body.h is this sequence, statement for statement, in double (the finite and the periodic VJP): a change
// to the step belongs in this file and in that header (one precision-generic body changes every kernel's text: DESIGN.md 3.26).
//
// Layout as lqr_steady_state_vjp.hip: every matrix of the step in the wave's LDS slice, every product on
// v_mfma_f32_16x16x4_f32 (wave_ops.h mfma_matmul, strict fp32).  NP = 16 serves n <= 16, NP = 32 serves n <= 32, both with
// m <= 16.  A gradient whose time stride is 0 is accumulated in the output in time order (a lane owns the same elements at
// every step); one whose batch stride is 0 is written as per-instance records into the workspace and summed by the shared
// batch sum (batch_sum.h: chunks of 256 instances, then the chunks in order).  A flagged instance (forward or here) gets NaN
// in its own rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/tfmpc_hip.h"
#include "batch_sum.h"
#include "tvlqr_kernels.h"
#include "wave_ops.h"

namespace tfmpc {

namespace {

constexpr int kMP = 16;                // controls per tile: m <= 16
constexpr int kRedChunk = 256;         // instances per stage-1 block of the batch sum
enum { kOutF, kOutf, kOutC, kOutc, kOutCf, kOutcf, kOuts };

struct BvOut {
    float *p;
    long sb, st;      // batch / time stride in elements (a workspace record when the caller's batch stride is 0)
};

struct BvArgs {
    int B, n, m, T;
    const float *F, *f, *C, *c;
    long sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t;
    const float *Cfin, *cfin;          // both NULL: the default final cost
    long sCfin_b, scfin_b;
    const float *K, *k, *V, *v;
    const int32_t *fwd_status;
    const float *gK, *gk, *gV, *gv, *gconst;
    BvOut o[kOuts];
    int32_t *status;
};

__device__ __forceinline__ void emit(const BvOut &o, int b, int t, int e, float x)
{
    float *p = o.p + (size_t)b * o.sb + (size_t)t * o.st + e;
    if (o.st == 0 && t > 0) x += *p;   // time-shared: accumulate in time order (this lane owns element e at every step)
    *p = x;
}

template <int NP>
__global__ __launch_bounds__(kWave) void tvb_vjp_kernel(BvArgs a)
{
    constexpr int DP = NP + kMP, LDN = NP + 1, LDD = DP + 1, LDA = kMP + NP + 3;
    __shared__ float sF[NP * LDD], sPF[NP * LDD], sT[NP * LDD], sQb[DP * LDD];
    __shared__ float sP[NP * LDN], sVb[NP * LDN], sK[kMP * LDN], sKV[kMP * LDN], sG[kMP * LDN], aug[kMP * LDA];
    __shared__ float vf[NP], vs[NP], vk[kMP], vvb[NP], vr[NP], vrb[NP], vq[DP], fac[kMP];

    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, T = a.T, d = n + m;
    const bool dflt = a.Cfin == nullptr;
    int status = a.fwd_status[b];
    float abar = 0.0f;
    auto zero = [](int, int) { return 0.0f; };
    const BvOut &oF = a.o[kOutF], &of = a.o[kOutf], &oC = a.o[kOutC], &oc = a.o[kOutc];

    wave_for_2d(n, n, [&](int i, int j, int) { sVb[i * LDN + j] = 0.0f; });
    for (int i = lane; i < n; i += kWave) vvb[i] = 0.0f;

    for (int t = 0; t < T && !status; ++t) {
        const size_t bt = (size_t)b * T + t;
        const bool last = t == T - 1;
        const float *Ft = tv_at(a.F, a.sF_b, a.sF_t, b, t), *ft = tv_at(a.f, a.sf_b, a.sf_t, b, t);
        const float *Cg = tv_at(a.C, a.sC_b, a.sC_t, b, t);
        // P = V_{t+1}, s = v_{t+1}; at the last step the final cost (default: C_{T-1}[:n,:n] with row stride d, c_{T-1}[:n])
        const float *Pg, *sg;
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
            if (a.gV) sVb[i * LDN + j] += 0.5f * (a.gV[bt * n * n + idx] + a.gV[bt * n * n + j * n + i]);
        });
        for (int i = lane; i < n; i += kWave) {
            vf[i] = ft[i];
            vs[i] = sg[i];
            if (a.gv) vvb[i] += a.gv[bt * n + i];
        }
        for (int r = lane; r < m; r += kWave) vk[r] = a.k[bt * m + r];
        // aug = [Quu | gK_t | gk_t]  (m rows)
        wave_for_2d(m, n + 1, [&](int r, int j, int) {
            aug[r * LDA + m + j] = j < n ? (a.gK ? a.gK[bt * m * n + r * n + j] : 0.0f) : (a.gk ? a.gk[bt * m + r] : 0.0f);
        });
        if (a.gconst) abar += a.gconst[bt];
        wsync();

        // PF = P F [n][d], KV = K Vbar [m][n], r = P f + s
        wave_matmul_mfma(n, d, n, [&](int i, int kk) { return sP[i * LDN + kk]; }, [&](int kk, int j) { return sF[kk * LDD + j]; },
                         zero, [&](int i, int j, float x) { sPF[i * LDD + j] = x; });
        wave_matmul_mfma(m, n, n, [&](int i, int kk) { return sK[i * LDN + kk]; }, [&](int kk, int j) { return sVb[kk * LDN + j]; },
                         zero, [&](int i, int j, float x) { sKV[i * LDN + j] = x; });
        wave_matvec(n, n, [&](int i, int j) { return sP[i * LDN + j]; }, [&](int j) { return vf[j]; },
                    [&](int i, float s) { vr[i] = s + vs[i]; });
        lds_sync();
        // Quu = C_uu + F_u' (P F)_u, symmetrised as in the forward
        wave_matmul_mfma(m, m, n, [&](int i, int kk) { return sF[kk * LDD + n + i]; }, [&](int kk, int j) { return sPF[kk * LDD + n + j]; },
                         [&](int i, int j) { return Cg[(n + i) * d + n + j]; }, [&](int i, int j, float x) { aug[i * LDA + j] = x; });
        wsync();
        symmetrise(aug, LDA, m);
        wsync();
        if (wave_gauss_jordan<false>(aug, LDA, m, m + n + 1, fac, fac)) {
            status |= TFMPC_ST_NOT_PD;
            break;
        }
        // G = KV + Kt [m][n];  qbar = [vbar; kt + K vbar + abar k]
        wave_for_2d(m, n, [&](int r, int j, int) { sG[r * LDN + j] = sKV[r * LDN + j] - aug[r * LDA + m + j]; });
        for (int i = lane; i < n; i += kWave) vq[i] = vvb[i];
        wave_matvec(m, n, [&](int r, int j) { return sK[r * LDN + j]; }, [&](int j) { return vvb[j]; },
                    [&](int r, float s) { vq[n + r] = fmaf(abar, vk[r], s - aug[r * LDA + m + n]); });
        lds_sync();
        // Qbar: the uu block (symmetrised below), xx = Vbar, ux / xu;  rbar = F qbar
        wave_matmul_mfma(m, m, n, [&](int i, int kk) { return sG[i * LDN + kk]; }, [&](int kk, int j) { return sK[j * LDN + kk]; },
                         [&](int i, int j) { return (vq[n + i] - 0.5f * abar * vk[i]) * vk[j]; },
                         [&](int i, int j, float x) { sQb[(n + i) * LDD + n + j] = x; });
        wave_for_2d(n, n, [&](int i, int j, int) { sQb[i * LDD + j] = sVb[i * LDN + j]; });
        wave_for_2d(m, n, [&](int r, int i, int) {
            const float x = 0.5f * (sKV[r * LDN + i] + sG[r * LDN + i] + vk[r] * vvb[i]);
            sQb[(n + r) * LDD + i] = x;
            sQb[i * LDD + n + r] = x;
        });
        wave_matvec(n, d, [&](int i, int j) { return sF[i * LDD + j]; }, [&](int j) { return vq[j]; }, [&](int i, float s) { vrb[i] = s; });
        lds_sync();
        symmetrise(sQb + n * LDD + n, LDD, m);
        lds_sync();
        // dF = 2 (PF) Qbar + r qbar';  T = F Qbar [n][d];  df = P rbar + abar r
        if (oF.p)
            wave_matmul_mfma(n, d, d, [&](int i, int kk) { return sPF[i * LDD + kk]; },
                             [&](int kk, int j) { return 2.0f * sQb[kk * LDD + j]; }, [&](int i, int j) { return vr[i] * vq[j]; },
                             [&](int i, int j, float x) { emit(oF, b, t, i * d + j, x); });
        wave_matmul_mfma(n, d, d, [&](int i, int kk) { return sF[i * LDD + kk]; }, [&](int kk, int j) { return sQb[kk * LDD + j]; },
                         zero, [&](int i, int j, float x) { sT[i * LDD + j] = x; });
        if (of.p)
            wave_matvec(n, n, [&](int i, int j) { return sP[i * LDN + j]; }, [&](int j) { return vrb[j]; },
                        [&](int i, float s) { emit(of, b, t, i, fmaf(abar, vr[i], s)); });
        lds_sync();
        // Vbar <- sym(T F' + rbar f' + abar f f' / 2) (through PF's tile), vbar <- rbar + abar f
        wave_matmul_mfma(n, n, d, [&](int i, int kk) { return sT[i * LDD + kk]; }, [&](int kk, int j) { return sF[j * LDD + kk]; },
                         [&](int i, int j) { return (vrb[i] + 0.5f * abar * vf[i]) * vf[j]; },
                         [&](int i, int j, float x) { sPF[i * LDD + j] = x; });
        lds_sync();
        wave_for_2d(n, n, [&](int i, int j, int) { sVb[i * LDN + j] = 0.5f * (sPF[i * LDD + j] + sPF[j * LDD + i]); });
        for (int i = lane; i < n; i += kWave) vvb[i] = fmaf(abar, vf[i], vrb[i]);
        lds_sync();
        // dC = Qbar, dc = qbar; the default final cost's gradient joins the last step's
        const bool fin = last && dflt;
        if (oC.p)
            wave_for_2d(d, d, [&](int i, int j, int idx) {
                float x = sQb[i * LDD + j];
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
            const int slots = (q < kOutCf && o.st) ? T : 1;
            for (int t = 0; t < slots; ++t) fill_nan(o.p + (size_t)b * o.sb + (size_t)t * o.st, sizes[q]);
        }
    }
    if (lane == 0) a.status[b] = status;
}

bool shape_supported(int n, int m) { return n <= 32 && m <= kMP; }

// the batch sum's workspace layout for the summed ones of dF, df, dC, dc (slots[q] = T or 1) and dCfin, dcfin
BatchSumPlan sum_plan(int B, int n, int m, const int slots[kOuts], unsigned summed)
{
    const int d = n + m;
    const int sizes[kOuts] = {n * d, n, d * d, d, n * n, n};
    return batch_sum_plan(B, kRedChunk, kOuts, sizes, slots, summed);
}

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

size_t tfmpc_tvlqr_backward_vjp_workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 1 || n <= 0 || m <= 0 || T <= 0 || !shape_supported(n, m)) return 0;
    const int slots[kOuts] = {T, T, T, T, 1, 1};
    return sum_plan(B, n, m, slots, (1u << kOuts) - 1).floats * sizeof(float);
}

const char *tfmpc_tvlqr_backward_vjp_kernel_name(int n, int m, int T)
{
    if (n <= 0 || m <= 0 || T <= 0) return "invalid";
    if (!shape_supported(n, m)) return "unsupported";
    if (n <= 16) return (n == 16 && (m == 8 || m == 16)) ? "tvb_vjp_mfma_16" : "tvb_vjp_mfma_16 (padded)";
    return "tvb_vjp_mfma_32";
}

int tfmpc_tvlqr_backward_vjp_f32(int B, int n, int m, int T,
                                 const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                                 const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                                 const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                                 const float *K, const float *k, const float *V, const float *v, const int32_t *fwd_status,
                                 const float *gK, const float *gk, const float *gV, const float *gv, const float *gconst,
                                 float *dF, long sdF_b, long sdF_t, float *df, long sdf_b, long sdf_t,
                                 float *dC, long sdC_b, long sdC_t, float *dc, long sdc_b, long sdc_t,
                                 float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b,
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
    float *outs[kOuts] = {dF, df, dC, dc, dCfin, dcfin};
    const long sb[kOuts] = {sdF_b, sdf_b, sdC_b, sdc_b, sdCfin_b, sdcfin_b};
    const long st[kOuts] = {sdF_t, sdf_t, sdC_t, sdc_t, 0, 0};
    // a batch stride of 0 sums over the batch
    int slots[kOuts];
    const unsigned summed = batch_sum_select(B, kOuts, outs, sb, st, T, slots);
    const BatchSumPlan plan = sum_plan(B, n, m, slots, summed);
    if (!plan.fits) return TFMPC_ERR_UNSUPPORTED;                  // the batch sum's blocks are one grid axis
    if (plan.floats && (!workspace || workspace_bytes < plan.floats * sizeof(float))) return TFMPC_ERR_WORKSPACE;
    float *w = static_cast<float *>(workspace);

    BvArgs a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = F; a.f = f; a.C = C; a.c = c;
    a.sF_b = sF_b; a.sF_t = sF_t; a.sf_b = sf_b; a.sf_t = sf_t; a.sC_b = sC_b; a.sC_t = sC_t; a.sc_b = sc_b; a.sc_t = sc_t;
    a.Cfin = Cfin; a.cfin = cfin; a.sCfin_b = sCfin_b; a.scfin_b = scfin_b;
    a.K = K; a.k = k; a.V = V; a.v = v; a.fwd_status = fwd_status;
    a.gK = gK; a.gk = gk; a.gV = gV; a.gv = gv; a.gconst = gconst;
    batch_sum_route(plan, w, outs, sb, st, [&](int q, float *p, long b, long t) { a.o[q] = {p, b, t}; });
    a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n <= 16) hipLaunchKernelGGL(tvb_vjp_kernel<16>, dim3(B), dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL(tvb_vjp_kernel<32>, dim3(B), dim3(kWave), 0, s, a);
    if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    return batch_sum_run<kRedChunk, kSumInOrder>(plan, w, outs, st, s);
}

}  // extern "C"
