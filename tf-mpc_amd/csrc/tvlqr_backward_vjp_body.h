// tvlqr_backward_vjp_body.h -- the ONE double-precision adjoint sweep of the Riccati recursion: the kernel template behind
// tfmpc_tvlqr_backward_vjp_f64 (tvlqr_backward_vjp_f64.hip, finite horizon) and the three sweeps of
// tfmpc_tvlqr_periodic_vjp_f64 (tvlqr_periodic_vjp_f64.hip, periodic infinite horizon).
//
// The sequence of tvlqr_backward_vjp.hip (fp32), statement for statement, in double -- a change to the
// step belongs in that file and in this header (one precision-generic body changed the text of all ten kernels: DESIGN.md
// 3.26).  Given the recursion's K_t, k_t, V_t, v_t and upstream gradients gK, gk, gV, gv, gconst, a wave sweeps FORWARD in
// time carrying the adjoints Vbar (n x n, symmetric), vbar (n) and abar (scalar) of V_t, v_t and const_t.  With P, s the
// value function after step t, step t is
//   Vbar += sym(gV_t), vbar += gv_t, abar += gconst_t
//   Quu = C_t,uu + F_t,u' P F_t,u;  [Kt | kt] = -Quu^-1 [gK_t | gk_t]   (elimination without pivoting: NOT_PD on a pivot <= 0)
//   qbar = [vbar; kt + K vbar + abar k]
//   Qbar_xx = Vbar,  Qbar_ux = (KV + G + k vbar') / 2,  Qbar_uu = sym(G K' + (qbar_u - abar k / 2) k'),  KV = K Vbar, G = KV + Kt
//   dC_t = Qbar, dc_t = qbar;  r = P f_t + s, rbar = F_t qbar;  dF_t = 2 (P F_t) Qbar + r qbar',  df_t = P rbar + abar r
//   Vbar <- sym(F_t Qbar F_t' + rbar f_t' + abar f_t f_t' / 2),  vbar <- rbar + abar f_t
// The propagation Vbar <- F Qbar F' is the closed loop A_cl Vbar A_cl', A_cl = F_x + F_u K: error does not compound with
// the horizon, which is why the fp32 sequence can be kept (unlike the costate recursion of DESIGN.md 3.15).
//
// The mode M (a struct of the including file) says what differs, and the body asks it with `if constexpr` at those places
// only:
//   M::Args        the kernel's argument struct (BvArgs / PvArgs: each stays in its file, member order untouched)
//   M::kPeriodic   false: one wave per instance sweeps t = 0 .. T-1 from the zero adjoint; P, s = V_{t+1}, v_{t+1}, at the
//                  last step the final cost, whose gradient is what leaves the sweep.  true: one wave per (instance,
//                  segment) sweeps its steps of the period; P, s = V_{(t+1) % N}, v_{(t+1) % N}; abar = 0 (no const output),
//                  and each abar-free expression is written out as such -- the periodic kernels' bits are those
//   M::kPass       kPassC writes dF, df, dC, dc (the finite sweep is a pass C); kPassA and kPassB of the periodic VJP only
//                  carry the adjoint, from (0, 0) with the running Psi <- A_cl Psi, and from (0, y_s)
//   M::steps(a)    T or N
// One __global__ template and no device function under two kernels: that changes the kernels' scalar code.
//
// Products run on v_mfma_f64_16x16x4_f64 (wave_ops_f64.h wave_matmul_f64<KMAX>, KMAX = NP or, where k = d, 2 NP),
// matrix-vector terms as fma() written out, the elimination and the rest on wave_ops.h's templates instantiated with
// double.  The LDS layout is the fp32 kernel's with m <= NP, carved from dynamic shared memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/tfmpc_hip.h"
#include "tvlqr_kernels.h"
#include "wave_ops_f64.h"

namespace tfmpc {

namespace {

using T = double;

enum { kOutF, kOutf, kOutC, kOutc, kOutCf, kOutcf };      // (dCfin, dcfin: the finite horizon's explicit final cost)
enum { kPassA, kPassB, kPassC };

struct BvOut {
    double *p;
    long sb, st;      // batch / time stride in elements (a workspace record when the caller's batch stride is 0)
};

__device__ __forceinline__ void emit(const BvOut &o, int b, int t, int e, double x)
{
    double *p = o.p + (size_t)b * o.sb + (size_t)t * o.st + e;
    if (o.st == 0 && t > 0) x += *p;   // time-shared: accumulate in time order (one wave; this lane owns element e at every step)
    *p = x;
}

// leading dimensions and element counts of the NP-wide LDS layout (the fp32 kernel's arrays with m <= NP): F, PF, T
// [NP][2 NP + 1] and Qbar [2 NP][2 NP + 1]; P, Vbar, K, KV, G [NP][NP + 1]; aug [NP][2 NP + 3]; nine NP-vectors (qbar
// takes two); pass A adds the running product Psi [NP][NP + 1]
template <int NP>
struct BvLayout {
    static constexpr int DP = 2 * NP, LDN = NP + 1, LDD = DP + 1, LDA = 2 * NP + 3;
    static constexpr int kWide = NP * LDD, kSq = NP * LDN, kAug = NP * LDA;
    static constexpr int kTotal = 5 * kWide + 5 * kSq + kAug + 9 * NP;
    static constexpr int total(int pass) { return kTotal + (pass == kPassA ? kSq : 0); }
};

// NP: the compile-time bound on n and m (16 or 32): the LDS tile width and the k-steps of every matrix product.
template <int NP, class M>
__global__ __launch_bounds__(kWave) void tvb_vjp_f64_kernel(typename M::Args a)
{
    using Lay = BvLayout<NP>;
    constexpr int LDN = Lay::LDN, LDD = Lay::LDD, LDA = Lay::LDA, WD = Lay::kWide, SQ = Lay::kSq;
    constexpr bool kPeriodic = M::kPeriodic;
    constexpr int PASS = M::kPass;
    extern __shared__ double tvb_vjp_smem_f64[];
    // the fp32 kernel's arrays, in its order, carved from dynamic shared memory
    T *const sF = tvb_vjp_smem_f64, *const sPF = sF + WD, *const sT = sPF + WD, *const sQb = sT + WD;
    T *const sP = sQb + 2 * WD, *const sVb = sP + SQ, *const sK = sVb + SQ, *const sKV = sK + SQ, *const sG = sKV + SQ;
    T *const aug = sG + SQ;
    T *const vf = aug + Lay::kAug, *const vs = vf + NP, *const vk = vs + NP, *const vvb = vk + NP, *const vr = vvb + NP;
    T *const vrb = vr + NP, *const vq = vrb + NP, *const fac = vq + 2 * NP;
    T *const sPsi = fac + NP;          // pass A only

    // the wave: instance b, and of the period segment seg = steps t0 .. t1-1 (block w)
    const size_t w = blockIdx.x;
    int b = blockIdx.x, seg = 0;
    if constexpr (kPeriodic) {
        b = (int)(blockIdx.x / (unsigned)a.segments);
        seg = (int)blockIdx.x - b * a.segments;
    }
    const int lane = lane_id();
    const int n = a.n, m = a.m, TT = M::steps(a), d = n + m;
    int t0 = 0, t1 = TT;
    int32_t *word = nullptr;           // the periodic sweep's status word
    int status = 0;
    bool dflt = false;
    if constexpr (kPeriodic) {
        t0 = seg * a.len;
        t1 = TT - t0 < a.len ? TT : t0 + a.len;
        word = (PASS == kPassA ? a.st_a : PASS == kPassB ? a.st_b : a.st_c) + w;
        // an instance that an earlier phase flagged is not swept
        if (PASS == kPassA ? a.fwd_status[b] : PASS == kPassB ? a.st_sa[b] : a.st_sb[b]) {
            if (lane == 0) *word = 0;
            return;
        }
    } else {
        dflt = a.Cfin == nullptr;
        status = a.fwd_status[b];
    }
    T abar = T(0);                     // (stays 0 and unread in the periodic sweeps)
    auto zero = [](int, int) { return T(0); };
    const BvOut &oF = a.o[kOutF], &of = a.o[kOutf], &oC = a.o[kOutC], &oc = a.o[kOutc];

    // the incoming adjoint: zero, or of the period (0, 0), (0, y_s) or (X_s, y_s), and Psi = I
    if constexpr (kPeriodic) {
        wave_for_2d(n, n, [&](int i, int j, int idx) {
            sVb[i * LDN + j] = PASS == kPassC ? a.Xs[w * n * n + idx] : T(0);
            if (PASS == kPassA) sPsi[i * LDN + j] = i == j ? T(1) : T(0);
        });
        for (int i = lane; i < n; i += kWave) vvb[i] = PASS == kPassA ? T(0) : a.ys[w * n + i];
    } else {
        wave_for_2d(n, n, [&](int i, int j, int) { sVb[i * LDN + j] = T(0); });
        for (int i = lane; i < n; i += kWave) vvb[i] = T(0);
    }

    for (int t = t0; t < t1 && (kPeriodic || !status); ++t) {
        const size_t bt = (size_t)b * TT + t;
        const bool last = !kPeriodic && t == TT - 1;
        const T *Ft = tv_at(a.F, a.sF_b, a.sF_t, b, t), *ft = tv_at(a.f, a.sf_b, a.sf_t, b, t);
        const T *Cg = tv_at(a.C, a.sC_b, a.sC_t, b, t);
        // P = V_{t+1}, s = v_{t+1}: the period wraps (V_N = V_0); the horizon ends with the final cost (default:
        // C_{T-1}[:n,:n] with row stride d, c_{T-1}[:n])
        const T *Pg, *sg;
        int ldP = n;
        if constexpr (kPeriodic) {
            const size_t bn = (size_t)b * TT + (t + 1 == TT ? 0 : t + 1);
            Pg = a.V + bn * n * n;
            sg = a.v + bn * n;
        } else if (!last) {
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
            sP[i * LDN + j] = kPeriodic ? Pg[idx] : Pg[i * ldP + j];
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
        if constexpr (!kPeriodic)
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
        wave_matvec<T>(m, n, [&](int r, int j) { return sK[r * LDN + j]; }, [&](int j) { return vvb[j]; }, [&](int r, T s) {
            if constexpr (kPeriodic) vq[n + r] = s - aug[r * LDA + m + n];
            else vq[n + r] = fma(abar, vk[r], s - aug[r * LDA + m + n]);
        });
        lds_sync();
        // Qbar: the uu block (symmetrised below), xx = Vbar, ux / xu;  rbar = F qbar
        wave_matmul_f64<NP>(m, m, n, [&](int i, int kk) { return sG[i * LDN + kk]; }, [&](int kk, int j) { return sK[j * LDN + kk]; },
                            [&](int i, int j) {
                                if constexpr (kPeriodic) return vq[n + i] * vk[j];
                                else return (vq[n + i] - T(0.5) * abar * vk[i]) * vk[j];
                            },
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
        if (PASS == kPassC && oF.p)
            wave_matmul_f64<2 * NP>(n, d, d, [&](int i, int kk) { return sPF[i * LDD + kk]; },
                                    [&](int kk, int j) { return T(2) * sQb[kk * LDD + j]; }, [&](int i, int j) { return vr[i] * vq[j]; },
                                    [&](int i, int j, T x) { emit(oF, b, t, i * d + j, x); });
        wave_matmul_f64<2 * NP>(n, d, d, [&](int i, int kk) { return sF[i * LDD + kk]; }, [&](int kk, int j) { return sQb[kk * LDD + j]; },
                                zero, [&](int i, int j, T x) { sT[i * LDD + j] = x; });
        if (PASS == kPassC && of.p)
            wave_matvec<T>(n, n, [&](int i, int j) { return sP[i * LDN + j]; }, [&](int j) { return vrb[j]; }, [&](int i, T s) {
                if constexpr (kPeriodic) emit(of, b, t, i, s);
                else emit(of, b, t, i, fma(abar, vr[i], s));
            });
        lds_sync();
        // Vbar <- sym(T F' + rbar f' + abar f f' / 2) (through PF's tile), vbar <- rbar + abar f
        wave_matmul_f64<2 * NP>(n, n, d, [&](int i, int kk) { return sT[i * LDD + kk]; }, [&](int kk, int j) { return sF[j * LDD + kk]; },
                                [&](int i, int j) {
                                    if constexpr (kPeriodic) return vrb[i] * vf[j];
                                    else return (vrb[i] + T(0.5) * abar * vf[i]) * vf[j];
                                },
                                [&](int i, int j, T x) { sPF[i * LDD + j] = x; });
        lds_sync();
        wave_for_2d(n, n, [&](int i, int j, int) { sVb[i * LDN + j] = T(0.5) * (sPF[i * LDD + j] + sPF[j * LDD + i]); });
        for (int i = lane; i < n; i += kWave) {
            if constexpr (kPeriodic) vvb[i] = vrb[i];
            else vvb[i] = fma(abar, vf[i], vrb[i]);
        }
        lds_sync();
        if constexpr (PASS == kPassC) {
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
        if constexpr (PASS == kPassA) {                                   // Psi <- A_cl Psi (through T's and PF's tiles)
            wave_matmul_f64<NP>(n, n, m, [&](int i, int kk) { return sF[i * LDD + n + kk]; }, [&](int kk, int j) { return sK[kk * LDN + j]; },
                                [&](int i, int j) { return sF[i * LDD + j]; }, [&](int i, int j, T x) { sT[i * LDD + j] = x; });
            lds_sync();
            wave_matmul_f64<NP>(n, n, n, [&](int i, int kk) { return sT[i * LDD + kk]; }, [&](int kk, int j) { return sPsi[kk * LDN + j]; },
                                zero, [&](int i, int j, T x) { sPF[i * LDD + j] = x; });
            lds_sync();
            wave_for_2d(n, n, [&](int i, int j, int) { sPsi[i * LDN + j] = sPF[i * LDD + j]; });
            lds_sync();
        }
    }

    if constexpr (kPeriodic) {
        if (!status) {                 // the outgoing adjoint
            if (PASS == kPassA) store_matrix(a.Psi + w * n * n, sPsi, LDN, n, n);
            else store_matrix(a.Ws + w * n * n, sVb, LDN, n, n);
            if (PASS != kPassB)
                for (int i = lane; i < n; i += kWave) a.sv[w * n + i] = vvb[i];
        }
        if (lane == 0) *word = status;
    } else {
        constexpr int kOuts = kOutcf + 1;
        const int sizes[kOuts] = {n * d, n, d * d, d, n * n, n};
        if (!status) {                 // the explicit final cost's gradient
            const BvOut &oCf = a.o[kOutCf], &ocf = a.o[kOutcf];
            if (oCf.p) wave_for_2d(n, n, [&](int i, int j, int idx) { oCf.p[(size_t)b * oCf.sb + idx] = sVb[i * LDN + j]; });
            if (ocf.p)
                for (int i = lane; i < n; i += kWave) ocf.p[(size_t)b * ocf.sb + i] = vvb[i];
        } else {                       // a flagged instance: NaN in its own rows
            for (int q = 0; q < kOuts; ++q) {
                const BvOut &o = a.o[q];
                if (!o.p) continue;
                const int slots = (q < kOutCf && o.st) ? TT : 1;
                for (int t = 0; t < slots; ++t) fill_nan(o.p + (size_t)b * o.sb + (size_t)t * o.st, sizes[q]);
            }
        }
        if (lane == 0) a.status[b] = status;
    }
}

}  // namespace

}  // namespace tfmpc
