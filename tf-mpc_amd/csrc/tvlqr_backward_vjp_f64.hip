// tvlqr_backward_vjp_f64.hip -- DOUBLE-PRECISION gradients of the finite-horizon Riccati recursion
// (tfmpc_tvlqr_backward_vjp_f64, include/tfmpc_hip.h): one wavefront per instance, n <= 32 and m <= 32.
//
// The adjoint step and its kernel template are tvlqr_backward_vjp_body.h's (shared with the periodic VJP,
// tvlqr_periodic_vjp_f64.hip).  This file is the FINITE mode: the wave sweeps t = 0 .. T-1 from the zero adjoint, carries
// abar (the adjoint of const_t) with Vbar and vbar, takes P = V_{t+1}, s = v_{t+1} and at t = T-1 the final cost, and writes
// every gradient as it goes.  After the last step Vbar, vbar are the final cost's gradient: dCfin, dcfin for an explicit
// final cost, added into dC_{T-1}[:n,:n], dc_{T-1}[:n] for the default one.
//
// LDS, carved from dynamic shared memory: 36.75 KiB for tvb_vjp_f64_wave16 (four waves per CU), 141.5 KiB for
// tvb_vjp_f64_wave32 (one; above the 64 KiB static limit, so the launch opts in to it).  A gradient whose time stride is 0
// is accumulated in the output in time order (a lane owns the same elements at every step); one whose batch stride is 0 is
// written as per-instance records into the workspace and summed by the shared batch sum in double (batch_sum.h: chunks of
// 64 instances, tree over the chunks).  A flagged instance (forward or here) gets NaN in its own rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/tfmpc_hip.h"
#include "batch_sum.h"
#include "launch.h"
#include "tvlqr_backward_vjp_body.h"

namespace tfmpc {

namespace {

constexpr int kRedChunk = 64;          // instances per stage-1 block of the batch sum
constexpr int kOuts = kOutcf + 1;      // dF, df, dC, dc, dCfin, dcfin

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

// the mode of tvb_vjp_f64_kernel (tvlqr_backward_vjp_body.h)
struct Finite {
    using Args = BvArgs;
    static constexpr bool kPeriodic = false;
    static constexpr int kPass = kPassC;
    static __device__ int steps(const BvArgs &a) { return a.T; }
};

static_assert(BvLayout<16>::kTotal == 4704 && BvLayout<32>::kTotal == 18112, "DESIGN.md 3.23: 36.75 KiB and 141.5 KiB");

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
    return launch_with_lds(tvb_vjp_f64_kernel<NP, Finite>, a.B, kWave, BvLayout<NP>::kTotal * sizeof(double), stream, a);
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
    // a batch stride of 0 sums over the batch
    int slots[kOuts];
    const unsigned summed = batch_sum_select(B, kOuts, outs, sb, st, T, slots);
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
    batch_sum_route(plan, w, outs, sb, st, [&](int q, double *p, long b, long t) { a.o[q] = {p, b, t}; });
    a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = wave16(n, m) ? launch_for<16>(a, s) : launch_for<32>(a, s);
    if (rc != TFMPC_OK) return rc;
    return batch_sum_run<kRedChunk, kSumTree, double>(plan, w, outs, st, s);
}

}  // extern "C"
