/* tfmpc_hip.h -- C ABI of the MI355X (gfx950) batched LQR / iLQR hot path.
 *
 * The reference (thiagopbueno/tf-mpc v0.7.0) is pure Python on TensorFlow and has
 * no FFI layer: its boundary is the Python class API of tfmpc/solvers/lqr.py and
 * tfmpc/solvers/ilqr.py.  Each entry point below names the reference method it
 * replaces (file:line in the reference tree); the Python host package
 * tf-mpc_amd/tfmpc binds them with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - All pointers are DEVICE pointers (hipMalloc / torch-ROCm storage), fp32,
 *    row-major, batch-major: the leading axis B indexes independent problem
 *    instances.  The library never allocates, frees or retains them.
 *  - A "batch stride" argument is the element distance between instances of that
 *    operand; 0 shares one copy between all instances.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *    only enqueue work; they never synchronise.
 *  - Return value: 0 on success, <0 on argument / launch error (TFMPC_ERR_*).
 *    Numerical trouble is reported per instance in `status[B]` (bit flags
 *    TFMPC_ST_*), never by aborting.
 *  - Scratch is passed in explicitly and sized by the *_workspace_bytes query.
 */
#ifndef TFMPC_HIP_H
#define TFMPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFMPC_OK 0
#define TFMPC_ERR_ARG (-1)         /* bad size / null pointer                          */
#define TFMPC_ERR_UNSUPPORTED (-2) /* shape exceeds what one wave's LDS tile can hold  */
#define TFMPC_ERR_LAUNCH (-3)      /* hipLaunchKernel reported an error                */
#define TFMPC_ERR_WORKSPACE (-4)   /* workspace too small                              */

#define TFMPC_ST_SINGULAR 0x1     /* LQR: zero pivot while inverting Q_uu (lqr.py:84)            */
#define TFMPC_ST_NOT_PD 0x2       /* iLQR: Cholesky of Q_uu_reg failed at least once (ilqr.py:305)*/
#define TFMPC_ST_NAN 0x4          /* a non-finite value reached an output                        */
#define TFMPC_ST_QP_MAXITER 0x8   /* box-QP hit its 100-iteration cap (optimization.py:13)       */
#define TFMPC_ST_MAX_ATTEMPTS 0x10 /* iLQR: backward/line-search attempt cap reached             */
#define TFMPC_ST_ENV_FLAG 0x40     /* TfmpcEnv::coupling_shift promised a chain that `downstream` is not: nothing was computed   */
#define TFMPC_ST_QP_LATER_NOT_PD 0x20 /* tfmpc_boxqp_f32: a factorisation AFTER the first failed; the loop broke out there as
                                         optimization.py:47-51 does: x and free are those at the break.  (Inside iLQR the QP starts at the box
                                         centre, ilqr.py:369, where every coordinate is free: the first factorisation is of the whole H, and a
                                         positive definite H has no indefinite principal block -- the case needs a boundary start or rounding.) */
#define TFMPC_ST_NOT_STABILISING 0x80 /* tfmpc_lqr_steady_state_f32: the doubling hit its cap, A_k did not go to zero, or a
                                          non-finite value appeared: no stabilising solution was found */

/* Library / device information ------------------------------------------------ */
int tfmpc_version(void);
/* Kernel-variant overrides for A/B timing and tests.  The environment variables TFMPC_LQR_KERNEL
 * (generic | lane | block), TFMPC_LQR_MFMA (f32 | bf16x3), TFMPC_ILQR_KERNEL (wave | lane | lane1 |
 * lean | lean1 | costate_mfma), TFMPC_LQR_WAVES (4 | 5 | 6: the register budget -- waves per SIMD -- of the headline LQR kernel's
 * instantiation; 6 exists for the launches without value outputs, the others then run at 5; same bits), TFMPC_COSTATE_WAVES (1 | 2 | 4 | 8: waves per sixteen-instance group of the HVAC /
 * Reservoir kernel; default: the form that brings the launch to about two waves per SIMD) and TFMPC_ILQR_RETRY (bracket: the control-limited LQ kernel looks for the regularisation level
 * of a failed factorisation around the level of its previous pass instead of probing 0, 1, 2, ... as ilqr.py:285-315
 * does -- another regularisation path on ~0.5 % of the instances; unsorted: that kernel launches its blocks in instance order instead of
 * starting the instances whose first backward pass probes most levels first -- same results, for A/B timing; levels: a batch whose sample shows no
 * such instance keeps instance order instead of starting its largest start costs first, as before round 6 -- same results; sorted: the whole batch is
 * probed whatever the sample says) and TFMPC_COSTATE_COUPLING
 * (dense: the 16-per-wave Reservoir kernel multiplies by its `downstream` matrix also when that matrix is a shift -- a chain of
 * reservoirs, every config the reference holds -- instead of moving rows; same bits, for A/B timing and tests), TFMPC_BOX_HELPERS (off | number of
 * helper teams, default 8: a control-limited batch of more than 4 096 instances without heavy ones in the launcher's sample lends five helper
 * blocks to each of its longest-running instances, which roll out the step sizes of a line search side by side -- same bits) and
 * TFMPC_BOX_HELP_AFTER (passes before an instance may claim a team, default 8), TFMPC_ILQR_LQ_REUSE (0: the matrix-core iLQR kernel of the
 * unbounded LQ env runs the full backward pass in every iteration, as ilqr.py:94-172 does; default: from the second pass on it keeps K_t and
 * Q_uu(t)^-1 -- which for a time-invariant LQ env at mu = 0 do not depend on the trajectory, so the recomputed ones would be the same bits -- and
 * runs only the vector recursion for k_t, V_x: results agree to fp32 rounding), TFMPC_GROUP_STORED (1 .. 4, default 4: how many step sizes of a
 * line search of the 2 x 2 lane-group kernel keep their candidate trajectory in the workspace; a pass that adopts another one rolls it out once
 * more -- same bits, for tests and A/B timing), TFMPC_BOX_SPECULATE (off | n, default 0: after n rejected passes in a row the helper team of a
 * control-limited instance runs the backward passes of its next passes beside its own -- same bits), TFMPC_TVLQR_TP_PHASES (1 | 2: tfmpc_tvlqr_solve_time_parallel_f64
 * returns TFMPC_TVLQR_TP_STOPPED (1, not TFMPC_OK) after its condense / its stitch launch and writes no output -- for timing the phases only; 1 .. 6: tfmpc_tvlqr_vjp_time_parallel_f64 likewise, after the launches its block lists) are read ONCE per process, at the first use of the library; afterwards only
 * this call changes them (value NULL or "" = back to the dispatcher's own choice).  Returns TFMPC_ERR_ARG
 * for an unknown name.  Process-wide; not meant to be flipped while other threads launch. */
int tfmpc_set_option(const char *name, const char *value);
/* The current override of `name` as a string in buf[len] ("" = none), so that a caller can restore what it replaces. */
int tfmpc_get_option(const char *name, char *buf, int len);
/* Name of the kernel variant the dispatcher would pick for an LQR shape
 * ("generic_wave", "mfma_16x8", ...).  Host-only; never touches the GPU. */
const char *tfmpc_lqr_kernel_name(int n, int m, int T);
/* Name of the kernel family the calling thread's LAST tfmpc_ilqr_solve_f32 / tfmpc_ilqr_solve_trace_f32 was dispatched to ("" before
 * the first).  A traced solve records its rows in the kernel that solves it; on HVAC / Reservoir and on the per-lane kernel of the
 * tiny 2-D envs that can be another kernel than the untraced solve takes (the LQ env's matrix-core kernels record their own trace
 * since round 4), which is what this call lets a caller report next to the trace (the CLI's -v writes it into trace.log). */
const char *tfmpc_ilqr_last_kernel_name(void);
/* Workgroups of the calling thread's last PERSISTENT lane-group launch (the 2-D envs of BASELINE configs[3] beyond 4 096 instances: the grid
 * is what the device holds at once for that launch's LDS size, and the groups pull instances from a queue); 0 before the first.  A
 * diagnostic: the grid must follow the horizon and the device of each launch, not those of the process's first launch. */
int tfmpc_ilqr_last_group_grid(void);

/* ---------------------------------------------------------------- LQR --------
 * Problem (tfmpc/solvers/lqr.py:18-57): x' = F [x;u] + f, stage cost
 * 1/2 z^T C z + c^T z, final cost 1/2 x^T C_xx x + c_x^T x, with
 * F[n][n+m], f[n], C[n+m][n+m], c[n+m].
 */

/* PRECONDITION of tfmpc_lqr_backward_f32 / _forward_f32 / _solve_f32: C is symmetric (every problem the
 * reference builds is: make_lqr draws make_spd_matrix, make_lqr_linear_navigation a diagonal,
 * tfmpc/envs/__init__.py:9-30).  The fast kernels use it: Q_xu is read as Q_ux^T, Q_uu is eliminated from its
 * upper triangle without pivoting (so Q_uu must be positive definite: C_uu > 0, C >= 0; a non-positive pivot
 * is reported as TFMPC_ST_NOT_PD / TFMPC_ST_SINGULAR) and V is kept exactly symmetric.  For a C that is NOT
 * symmetric the reference's recursion (lqr.py:74-105: Q_ux and Q_xu separately, tf.linalg.inv, four-term
 * update, no symmetrisation) gives a different answer than any symmetrised solve; call the *_general_f32
 * twins below, which restate it term by term on the wave-per-instance kernel (same arguments, any C).
 * The Python class checks C once at construction and picks the entry points accordingly. */

/* Bytes of scratch tfmpc_lqr_solve_f32 needs when K / k are not requested as
 * outputs (the gains are kept for the forward pass). */
size_t tfmpc_lqr_workspace_bytes(int B, int n, int m, int T);

/* LQR.backward (lqr.py:59-129): Riccati recursion from V=C_xx, v=c_x.
 * Outputs (each may be NULL except K, k): K[B][T][m][n], k[B][T][m],
 * V[B][T][n][n], v[B][T][n], cst[B][T] -- entry t is time t, the terminal entry
 * is dropped as in lqr.py:126-127.  status[B] may be NULL. */
int tfmpc_lqr_backward_f32(int B, int n, int m, int T,
                           const float *F, long strideF, const float *f, long stride_f,
                           const float *C, long strideC, const float *c, long stride_c,
                           float *K, float *k, float *V, float *v, float *cst,
                           int32_t *status, void *stream);

/* LQR.forward (lqr.py:131-161): u_t = K_t x_t + k_t, rollout and costs.
 * K[B][T][m][n] (batch stride strideK, 0 = shared policy), k likewise.
 * Outputs states[B][T+1][n], actions[B][T][m], costs[B][T+1]. */
int tfmpc_lqr_forward_f32(int B, int n, int m, int T,
                          const float *F, long strideF, const float *f, long stride_f,
                          const float *C, long strideC, const float *c, long stride_c,
                          const float *K, long strideK, const float *k, long stride_k,
                          const float *x0,
                          float *states, float *actions, float *costs, void *stream);

/* LQR.solve (lqr.py:163-166): backward + forward fused in one launch.
 * K, k, V, v, cst are optional outputs (NULL to skip).  If K or k is NULL,
 * `workspace` must hold tfmpc_lqr_workspace_bytes(...) bytes. */
int tfmpc_lqr_solve_f32(int B, int n, int m, int T,
                        const float *F, long strideF, const float *f, long stride_f,
                        const float *C, long strideC, const float *c, long stride_c,
                        const float *x0,
                        float *states, float *actions, float *costs,
                        float *K, float *k, float *V, float *v, float *cst,
                        int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* The policy (K_t, k_t) and the value function (V_t, v_t, const_t) of lqr.py:107-129 in 16-BIT containers (SURVEY.md 8f
 * N4: they are 9 x the bytes of the trajectory -- 81.8 KB per solve at n = 16, m = 8, T = 50, 40.9 KB like this).
 * K16, k16, V16, v16, cst16: bf16 arrays (uint16_t) in the layouts of K, k, V, v, cst, any may be NULL; every value is
 * the fp32 result rounded to nearest even, i.e. exactly what rounding tfmpc_lqr_solve_f32's outputs would give.  The
 * trajectory (states, actions, costs: fp32) is rolled out with the fp32 gains and is identical to
 * tfmpc_lqr_solve_f32's.  `workspace`: tfmpc_lqr_workspace_bytes (the fp32 gains live there).  Shapes the lane /
 * workgroup kernels serve go to the wave kernel; TFMPC_ERR_UNSUPPORTED beyond its LDS limit (n = m ~ 48). */
int tfmpc_lqr_solve_bf16out_f32(int B, int n, int m, int T,
                                const float *F, long strideF, const float *f, long stride_f,
                                const float *C, long strideC, const float *c, long stride_c,
                                const float *x0,
                                float *states, float *actions, float *costs,
                                uint16_t *K16, uint16_t *k16, uint16_t *V16, uint16_t *v16, uint16_t *cst16,
                                int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
/* LQR.backward alone, 16-bit outputs (same contract; `workspace` as above). */
int tfmpc_lqr_backward_bf16out_f32(int B, int n, int m, int T,
                                   const float *F, long strideF, const float *f, long stride_f,
                                   const float *C, long strideC, const float *c, long stride_c,
                                   uint16_t *K16, uint16_t *k16, uint16_t *V16, uint16_t *v16, uint16_t *cst16,
                                   int32_t *status, void *workspace, size_t workspace_bytes, void *stream);


/* The same three calls for a C that is not symmetric (see PRECONDITION above). */
int tfmpc_lqr_backward_general_f32(int B, int n, int m, int T,
                                   const float *F, long strideF, const float *f, long stride_f,
                                   const float *C, long strideC, const float *c, long stride_c,
                                   float *K, float *k, float *V, float *v, float *cst,
                                   int32_t *status, void *stream);
int tfmpc_lqr_forward_general_f32(int B, int n, int m, int T,
                                  const float *F, long strideF, const float *f, long stride_f,
                                  const float *C, long strideC, const float *c, long stride_c,
                                  const float *K, long strideK, const float *k, long stride_k,
                                  const float *x0,
                                  float *states, float *actions, float *costs, void *stream);
int tfmpc_lqr_solve_general_f32(int B, int n, int m, int T,
                                const float *F, long strideF, const float *f, long stride_f,
                                const float *C, long strideC, const float *c, long stride_c,
                                const float *x0,
                                float *states, float *actions, float *costs,
                                float *K, float *k, float *V, float *v, float *cst,
                                int32_t *status, void *workspace, size_t workspace_bytes, void *stream);


/* ------------------------------------------------------- time-varying LQR --------
 * TV-LQR: the problem above with a model per step.  For each instance b, z_t = [x_t; u_t], d = n + m:
 *   x_{t+1} = F_t z_t + f_t,  F_t[n][d], f_t[n];  stage cost 1/2 z_t^T C_t z_t + c_t^T z_t,  C_t[d][d], c_t[d];
 *   final cost 1/2 x_T^T C_fin x_T + c_fin^T x_T,  Cfin[n][n], cfin[n].
 * Model operand X of instance b at step t is read at X + b * sX_b + t * sX_t (elements): sX_b = 0 shares it across
 * the batch, sX_t = 0 holds it constant in time.  Cfin / cfin have a batch stride only; both NULL selects
 * C_fin = C_{T-1}[:n,:n], c_fin = c_{T-1}[:n] (with every step equal: exactly tfmpc_lqr_*_f32's problem).
 * T >= 1.  Backward: the recursion of tfmpc_lqr_backward_f32 with F_t, f_t, C_t, c_t at step t (const accumulates
 * with f_t and the value function of step t+1).  Outputs, statuses and error codes as in the LQR block, including
 * the PRECONDITION (C_t and C_fin symmetric, C_t,uu > 0: TFMPC_ST_NOT_PD / TFMPC_ST_SINGULAR per instance).
 * n <= 16, m <= 8: the 16 x 8 matrix-core sweep (models streamed per step); larger shapes: a wave-per-instance
 * fp32 kernel up to its LDS limit, TFMPC_ERR_UNSUPPORTED beyond.  B == 0 is a no-op. */
size_t tfmpc_tvlqr_workspace_bytes(int B, int n, int m, int T);
const char *tfmpc_tvlqr_kernel_name(int n, int m, int T);
int tfmpc_tvlqr_backward_f32(int B, int n, int m, int T,
                             const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                             const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                             const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                             float *K, float *k, float *V, float *v, float *cst, int32_t *status, void *stream);
/* K[B][T][m][n] with batch stride strideK (0 = one policy for the batch), k likewise. */
int tfmpc_tvlqr_forward_f32(int B, int n, int m, int T,
                            const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                            const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                            const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                            const float *K, long strideK, const float *k, long stride_k,
                            const float *x0, float *states, float *actions, float *costs, void *stream);
/* Fused backward + forward; K, k, V, v, cst optional (if K or k is NULL, `workspace` must hold
 * tfmpc_tvlqr_workspace_bytes(...) bytes). */
int tfmpc_tvlqr_solve_f32(int B, int n, int m, int T,
                          const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                          const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                          const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                          const float *x0, float *states, float *actions, float *costs,
                          float *K, float *k, float *V, float *v, float *cst, int32_t *status,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------------- time-varying LQR, double precision --------
 * The TV-LQR block above with every value a double: the same problem, operand strides (in elements),
 * outputs, statuses, error codes and B == 0 no-op; status stays int32.  One wavefront per instance, the three matrix
 * products of a step on v_mfma_f64_16x16x4_f64, for n <= 32 and m <= 32 (kernel_name_f64: "tv_f64_wave16" for n <= 16
 * and m <= 16, "tv_f64_wave32" otherwise); beyond: TFMPC_ERR_UNSUPPORTED ("unsupported").  The split backward + forward
 * calls give the bits of the fused solve.  workspace_bytes_f64 = B T m (n + 1) 8.  Gradients: tfmpc_tvlqr_vjp_f64 below. */
size_t tfmpc_tvlqr_workspace_bytes_f64(int B, int n, int m, int T);
const char *tfmpc_tvlqr_kernel_name_f64(int n, int m, int T);
int tfmpc_tvlqr_backward_f64(int B, int n, int m, int T,
                             const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                             const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                             const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                             double *K, double *k, double *V, double *v, double *cst, int32_t *status, void *stream);
int tfmpc_tvlqr_forward_f64(int B, int n, int m, int T,
                            const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                            const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                            const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                            const double *K, long strideK, const double *k, long stride_k,
                            const double *x0, double *states, double *actions, double *costs, void *stream);
int tfmpc_tvlqr_solve_f64(int B, int n, int m, int T,
                          const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                          const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                          const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                          const double *x0, double *states, double *actions, double *costs,
                          double *K, double *k, double *V, double *v, double *cst, int32_t *status,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------- time-varying LQR, double precision, time-parallel --------
 * tfmpc_tvlqr_solve_f64's problem with the horizon cut into segments that are worked on concurrently:
 * for a FEW LONG horizons (B <= 64 or so, T in the hundreds or thousands), where one wavefront per instance leaves the
 * card idle.  `segments` is clamped to T; every segment has len = ceil(T / segments) steps but a shorter last one, and
 * there are P = ceil(T / len) of them.  Three phases, each one kernel: condense (one wave per instance and segment
 * reduces its steps to one segment element), stitch (one wave per instance: the value function at every segment's end,
 * then the state at every segment's start), expand (one wave per instance and segment: tfmpc_tvlqr_solve_f64's own
 * recursion and rollout on the segment); a fourth, small kernel ORs the status words.  The result is the solution of the
 * same problem, NOT the bits of tfmpc_tvlqr_solve_f64 (the value function crosses a segment boundary by another formula);
 * with P == 1 the call forwards to tfmpc_tvlqr_solve_f64 and returns its bits.
 * Arguments: tfmpc_tvlqr_solve_f64's, with `segments` after `status`; the same operand strides (0 included), final cost,
 * optional K, k, V, v and the same checks in the same order, then: segments < 1 or cst != NULL is TFMPC_ERR_ARG (the
 * value function's constant term is not carried through the elements).  The workspace is always required for P > 1:
 * with w = B P,  8 (w (4 n n + 4 n) + B T m (n + 1)) + the bytes of 2 w + B status words rounded up to 8
 * (workspace_bytes_f64(B, n, m, T, segments); 0 for an invalid argument); a workspace that is not 8-byte aligned is
 * TFMPC_ERR_ARG.
 * status[b] is the OR over the instance's segments and its stitch: TFMPC_ST_NOT_PD for a step's R_t = C_t[n:,n:] or
 * Q_uu not positive definite, TFMPC_ST_SINGULAR for a singular I + G H at a combine or boundary, TFMPC_ST_NAN as the
 * sequential solve; a flagged instance has NaN in all its outputs.  No atomics: an instance's bits depend on neither B
 * nor its position, and repeated calls give identical bits.  kernel_name: "tv_f64_time_parallel16" (n <= 16 and
 * m <= 16) or "tv_f64_time_parallel32", the sequential kernel's name when P == 1, "unsupported", "invalid". */
#define TFMPC_TVLQR_TP_STOPPED 1    /* stopped after a phase on request (TFMPC_TVLQR_TP_PHASES): no output was written */
size_t tfmpc_tvlqr_time_parallel_workspace_bytes_f64(int B, int n, int m, int T, int segments);
const char *tfmpc_tvlqr_time_parallel_kernel_name_f64(int n, int m, int T, int segments);
int tfmpc_tvlqr_solve_time_parallel_f64(int B, int n, int m, int T,
                                        const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                                        const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                                        const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                                        const double *x0, double *states, double *actions, double *costs,
                                        double *K, double *k, double *V, double *v, double *cst, int32_t *status,
                                        int segments, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------- periodic infinite-horizon LQR, double precision --------
 * The infinite-horizon problem whose model repeats with period N: F, f, C, c are ONE PERIOD, with
 * tfmpc_tvlqr_solve_f64's operand layout and strides (0 allowed on either axis; a time stride of 0 with N > 1 is the
 * stationary problem sampled N times); there is no final cost and no x0.  Outputs, each optional: the periodic stabilising
 * gains K[B][N][m][n], k[B][N][m] and value function V[B][N][n][n], v[B][N][n], V[b][t], v[b][t] AT step t as
 * tfmpc_tvlqr_backward_f64's (V[b][0] = P_0; V_N = V_0, v_N = v_0); residual[B] (optional): one more turn around the period
 * from (P_0, p_0), max(max|V - P_0| / max|P_0|, max|v - p_0| / max(1, max|p_0|)), a self-check; iterations[B]
 * (optional): doubling steps taken; status[B] (required).
 * Four kernels on the caller's stream: the time-parallel solve's condense on the period's segments (`segments` clamped
 * to N: len = ceil(N / segments), P = ceil(N / len)); a stitch, one wave per instance, that folds the P elements into
 * the one-period element, doubles it -- the element of 2^k periods: H_k -> P_0, h_k -> p_0, A_k -> 0 -- until
 * max|H_k - H_{k-1}| <= tol max|H_k|, max|h_k - h_{k-1}| <= tol max(1, max|h_k|) and max|A_k| <= 1e-3, certifies the
 * closed-loop monodromy (I + G1 P_0)^-1 A1 by squaring it below 1e-3 within max_iter squarings, and carries (P_0, p_0)
 * backwards over the seams; an expand, one wave per (instance, segment), that runs tfmpc_tvlqr_backward_f64's recursion
 * on its segment; a finish that ORs the status words.  max_iter 0 -> 40, tol 0 -> 4 DBL_EPSILON.
 * Checks: tfmpc_tvlqr_solve_time_parallel_f64's on the model, in its order (n > 32 or m > 32: TFMPC_ERR_UNSUPPORTED), then
 * segments < 1, max_iter < 0 or tol < 0: TFMPC_ERR_ARG; B == 0 is a no-op; status == NULL, a workspace that is NULL,
 * smaller than workspace_bytes or not 8-byte aligned: TFMPC_ERR_ARG.  The workspace is always required: with w = B P,
 *   8 ((w + B) (3 n n + 2 n) + w (n n + n) + B N m (n + 1)) + the bytes of 2 w + B status words rounded up to 8
 * (the segment and the one-period elements, the value behind every segment, the gains; 0 for an invalid argument).
 * status[b]: TFMPC_ST_NOT_PD for a step's R_t or Q_uu not positive definite, TFMPC_ST_SINGULAR for a zero pivot in any
 * I + G H, I + P G or I + G P, TFMPC_ST_NOT_STABILISING when the doubling meets a non-finite value or does not stop within
 * max_iter steps or the certificate fails, TFMPC_ST_NAN as the sequential solve.  A phase does not run on an instance an
 * earlier phase flagged, so the word names the cause.  A flagged instance has NaN in all its outputs (iterations keeps
 * its count); no other instance is affected.  No atomics, no allocation, no sync: an instance's bits depend on neither B
 * nor its position, and repeated calls give identical bits.  kernel_name: "tv_f64_periodic16" (n <= 16 and m <= 16) or
 * "tv_f64_periodic32", "unsupported", "invalid".  TFMPC_TVLQR_TP_PHASES = 1 | 2 | 3 stops the call after its condense /
 * stitch / expand launch (TFMPC_TVLQR_TP_STOPPED; timing only). */
size_t tfmpc_tvlqr_periodic_workspace_bytes_f64(int B, int n, int m, int N, int segments);
const char *tfmpc_tvlqr_periodic_kernel_name_f64(int n, int m, int N, int segments);
int tfmpc_tvlqr_periodic_steady_state_f64(int B, int n, int m, int N,
                                          const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                                          const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                                          int segments, int max_iter, double tol,
                                          double *K, double *k, double *V, double *v, double *residual,
                                          int32_t *iterations, int32_t *status,
                                          void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------ TV-LQR gradients --------
 * Vector-Jacobian product of tfmpc_tvlqr_solve_f32: given the forward's states[B][T+1][n] (states[b][0]
 * is x0) and actions[B][T][m], and upstream gradients g_states[B][T+1][n], g_actions[B][T][m], g_costs[B][T+1] (each
 * NULL = zero), writes the gradients of sum(g_states * states) + sum(g_actions * actions) + sum(g_costs * costs) with
 * respect to F, f, C, c, Cfin, cfin and x0.  Model operands and their strides as in tfmpc_tvlqr_solve_f32 (Cfin = cfin =
 * NULL: the default final cost, whose gradient then lands in dC[T-1][:n,:n] and dc[T-1][:n]; dCfin / dcfin must be NULL).
 * Every output has its own batch and time stride in elements (dCfin, dcfin, dx0: batch only); a stride of 0 SUMS the
 * gradient over that axis.  A NULL output is not computed.  C and Cfin enter as symmetric matrices, so dC and dCfin are
 * the symmetric gradients.  The reductions run in a fixed order without atomics: repeated calls give identical bits.
 * status[B] (required) gets the adjoint solve's status; an instance with TFMPC_ST_NOT_PD or TFMPC_ST_SINGULAR has NaN
 * in its own gradient rows and in every batch-summed gradient.  workspace must hold
 * tfmpc_tvlqr_vjp_workspace_bytes(B, n, m, T) bytes.  Shapes as the solve serves; B == 0 is a no-op. */
size_t tfmpc_tvlqr_vjp_workspace_bytes(int B, int n, int m, int T);
int tfmpc_tvlqr_vjp_f32(int B, int n, int m, int T,
                        const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                        const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                        const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                        const float *states, const float *actions,
                        const float *g_states, const float *g_actions, const float *g_costs,
                        float *dF, long sdF_b, long sdF_t, float *df, long sdf_b, long sdf_t,
                        float *dC, long sdC_b, long sdC_t, float *dc, long sdc_b, long sdc_t,
                        float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b, float *dx0, long sdx0_b,
                        int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------- TV-LQR gradients, double precision --------
 * Vector-Jacobian product of tfmpc_tvlqr_solve_f64: tfmpc_tvlqr_vjp_f32's contract with every value a
 * double (strides in elements, NULL upstream = zero, a NULL output is not computed, a stride of 0 sums over that axis in a
 * fixed order without atomics so that repeated calls give identical bits, the default final cost's gradient in dC[T-1],
 * dc[T-1], dCfin / dcfin without Cfin is TFMPC_ERR_ARG, B == 0 is a no-op, error codes before any launch).  One more
 * input is REQUIRED: v[B][T][n], the forward solve's value-gradient term (call tfmpc_tvlqr_solve_f64 with v non-NULL).
 * The costates are the value function's gradient on the optimal trajectory, lam_t = V_t x_t + v_t and
 * dlam_t = V_t dx_t + v~_t with V, v~ from the adjoint solve: closed-loop, so rounding error does not grow with the
 * horizon as it does in the f32 call's open-loop costate recursion.  Shapes as the f64 solve serves (n <= 32, m <= 32;
 * beyond: TFMPC_ERR_UNSUPPORTED).  status[B] (required) gets the adjoint solve's status; an instance with any bit set has
 * NaN in its own gradient rows and in every batch-summed gradient.  With up(x) = x rounded up to a multiple of 64,
 * d = n + m and chunks = ceil(B / 256), the workspace holds
 *   8 * [ up(B T d) + 2 up(B n) + up(B n n) + up(B (T+1) n) + up(B T m) + up(B (T+1)) + up(B T m (n+1))
 *         + up(B T n n) + up(B T n) + up(2 B T n) + up(chunks T (n d + n + d d + d)) ]  bytes
 * (fold, adjoint trajectory, the solve's gains, the adjoint's V and v~, the costate records, the partial sums): the V
 * field alone is 6.7 GB at B = 65536, n = 16, T = 50. */
size_t tfmpc_tvlqr_vjp_workspace_bytes_f64(int B, int n, int m, int T);
int tfmpc_tvlqr_vjp_f64(int B, int n, int m, int T,
                        const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                        const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                        const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                        const double *states, const double *actions, const double *v,
                        const double *g_states, const double *g_actions, const double *g_costs,
                        double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                        double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t,
                        double *dCfin, long sdCfin_b, double *dcfin, long sdcfin_b, double *dx0, long sdx0_b,
                        int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------- TV-LQR gradients, double precision, time-parallel (segmented adjoint) --------
 * tfmpc_tvlqr_vjp_f64's contract and argument order for a FEW LONG horizons, the companion of
 * tfmpc_tvlqr_solve_time_parallel_f64.  Two more inputs are REQUIRED beside v: the forward's K[B][T][m][n] and
 * V[B][T][n][n] (that solve writes both on request).  The adjoint problem has the forward's F, C, C_fin, hence its gains
 * and value function; its vector part is two affine recursions in the closed-loop transition Phi_t = F_t [I; K_t], which
 * are condensed per segment to one n x n matrix and one offset per direction, stitched with P matrix-vector products
 * and expanded concurrently.  No Riccati step is repeated; the only elimination is Q_uu,t = C_t[n:,n:] + B_t' V_{t+1} B_t,
 * without pivoting, once per (b, t).  `segments` follows `status`: clamped to T, len = ceil(T / segments),
 * P = ceil(T / len) as in tfmpc_tvlqr_solve_time_parallel_f64.  With P == 1 the call forwards to tfmpc_tvlqr_vjp_f64,
 * ignores K and V and returns its bits (and that call's workspace rule applies).
 * Checks, before any launch: tfmpc_tvlqr_vjp_f64's in its order, with segments < 1 (TFMPC_ERR_ARG) after the shape
 * tests and K or V NULL (TFMPC_ERR_ARG, P > 1) after v; a workspace that is not 8-byte aligned is TFMPC_ERR_ARG.
 * status[b] is the OR over the instance's steps: TFMPC_ST_NOT_PD for a non-positive pivot of Q_uu,t; an instance with any
 * bit set has NaN in its own gradient rows and in every batch-summed gradient.  No atomics, every sum in a fixed order:
 * an instance's bits depend on neither B nor its position, and repeated calls give identical bits.  A per-instance
 * output with time stride 0 is accumulated by tfmpc_tvlqr_vjp_f64's one-wave-per-instance costate walk, which stays
 * serial in T.  With up(x) = x rounded up to a multiple of 64, d = n + m, chunks = ceil(B / 256), the workspace for P > 1
 * holds
 *   8 * [ up(B T d) + 2 up(B n) + up(B n n) + up(B (T+1) n) + up(B T m) + up(B (T+1))
 *         + up(B T n n) + up(B T n) + up(B T m) + up(B T n m) + up(B T n) + up(B T n) + up(2 B T n)
 *         + up(chunks T (n d + n + d d + d)) + up(B P n n) + 4 up(B P n) + up(ceil(B T / 2)) ]  bytes
 * (fold and adjoint trajectory; Phi, a, r, E, w per step; v~; the costate records; the partial sums; M, beta, gamma and
 * the boundary vectors per segment; one status word per step): no V, no gains and no solve workspace of its own.
 * TFMPC_TVLQR_TP_PHASES = 1 .. 6 stops this call after the step kernel / the condense / the backward stitch / the
 * backward expand / the forward stitch / the forward expand (TFMPC_TVLQR_TP_STOPPED, no output written; timing only). */
size_t tfmpc_tvlqr_vjp_time_parallel_workspace_bytes_f64(int B, int n, int m, int T, int segments);
int tfmpc_tvlqr_vjp_time_parallel_f64(int B, int n, int m, int T,
                                      const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                                      const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                                      const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                                      const double *states, const double *actions, const double *v,
                                      const double *K, const double *V,
                                      const double *g_states, const double *g_actions, const double *g_costs,
                                      double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                                      double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t,
                                      double *dCfin, long sdCfin_b, double *dcfin, long sdcfin_b, double *dx0, long sdx0_b,
                                      int32_t *status, int segments, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------- gradients of the Riccati recursion --------
 * Vector-Jacobian product of tfmpc_tvlqr_backward_f32: given the recursion's K[B][T][m][n], k[B][T][m],
 * V[B][T][n][n], v[B][T][n] and status[B] (fwd_status), and upstream gradients gK, gk, gV, gv, gconst[B][T] of the same
 * layouts (each NULL = zero), writes the gradients of <gK, K> + <gk, k> + <gV, V> + <gv, v> + <gconst, const> with
 * respect to F, f, C, c, Cfin and cfin.  Model operands, strides and the final cost as in tfmpc_tvlqr_backward_f32
 * (Cfin = cfin = NULL: the default final cost, whose gradient then lands in dC[T-1][:n,:n] and dc[T-1][:n]; dCfin / dcfin
 * must be NULL).  One sweep forward in time carries the adjoints of V_t, v_t, const_t; it reads the model and K, k, V, v
 * only (the recursion is not recomputed) and eliminates Q_uu = C_t,uu + F_t,u' V_{t+1} F_t,u once per step without
 * pivoting (a non-positive pivot: TFMPC_ST_NOT_PD).  Outputs, their batch and time strides, stride-0 sums (time: in the
 * sweep, in time order; batch: per-instance records in the workspace and a fixed-order two-stage sum, no atomics --
 * repeated calls give identical bits), NULL outputs and the symmetric dC, dCfin as in tfmpc_tvlqr_vjp_f32.  status[B]
 * (required) gets the forward's status where it was flagged, else this sweep's; a flagged instance has NaN in its own
 * gradient rows and in every batch-summed gradient.  workspace: tfmpc_tvlqr_backward_vjp_workspace_bytes(B, n, m, T) bytes
 * serve any choice of summed outputs (NULL is fine when no output is summed over a batch of more than one).
 * n <= 16, m <= 16: 16-wide LDS tiles; n <= 32, m <= 16: 32-wide; beyond: TFMPC_ERR_UNSUPPORTED (kernel_name:
 * "unsupported").  One wave per instance, every product on the f32 matrix cores.  B == 0 is a no-op. */
size_t tfmpc_tvlqr_backward_vjp_workspace_bytes(int B, int n, int m, int T);
const char *tfmpc_tvlqr_backward_vjp_kernel_name(int n, int m, int T);
int tfmpc_tvlqr_backward_vjp_f32(int B, int n, int m, int T,
                                 const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                                 const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                                 const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                                 const float *K, const float *k, const float *V, const float *v, const int32_t *fwd_status,
                                 const float *gK, const float *gk, const float *gV, const float *gv, const float *gconst,
                                 float *dF, long sdF_b, long sdF_t, float *df, long sdf_b, long sdf_t,
                                 float *dC, long sdC_b, long sdC_t, float *dc, long sdc_b, long sdc_t,
                                 float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b,
                                 int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* tfmpc_tvlqr_backward_vjp_f32 in double, for the K, k, V, v of tfmpc_tvlqr_backward_f64: the same
 * sweep, argument rules, strides, stride-0 sums, status bits and NaN rows, every operand, upstream gradient and output
 * double, products on the f64 matrix cores.  The batch sum runs in double over chunks of 64 instances, then a tree over
 * the chunks (the order of tfmpc_lqr_steady_state_vjp_f64).  n <= 16, m <= 16: "tvb_vjp_f64_wave16"; n <= 32, m <= 32:
 * "tvb_vjp_f64_wave32" (141.5 KiB of dynamic LDS, one wave per CU); beyond: TFMPC_ERR_UNSUPPORTED.  workspace:
 * tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(B, n, m, T) bytes (the plan's element counts, 8 bytes each). */
size_t tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(int B, int n, int m, int T);
const char *tfmpc_tvlqr_backward_vjp_kernel_name_f64(int n, int m, int T);
int tfmpc_tvlqr_backward_vjp_f64(int B, int n, int m, int T,
                                 const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                                 const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                                 const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                                 const double *K, const double *k, const double *V, const double *v, const int32_t *fwd_status,
                                 const double *gK, const double *gk, const double *gV, const double *gv, const double *gconst,
                                 double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                                 double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t,
                                 double *dCfin, long sdCfin_b, double *dcfin, long sdcfin_b,
                                 int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------- periodic infinite-horizon LQR gradients, double precision --------
 * Vector-Jacobian product of tfmpc_tvlqr_periodic_steady_state_f64: given the model of ONE PERIOD with
 * its strides as in the forward, the forward's K[B][N][m][n], k[B][N][m], V[B][N][n][n], v[B][N][n] and status
 * (fwd_status[B], required) and upstream gradients gK, gk, gV, gv in the shapes of K, k, V, v (each optional, NULL = zero),
 * the gradients dF[n][d], df[n], dC[d][d] (symmetric), dc[d] per (b, t), each optional, each with a batch and a time stride
 * in elements as in tfmpc_tvlqr_backward_vjp_f64.  The step is that entry's with P = V[(t + 1) % N]; the period has no
 * final cost, so the adjoint (X, y) of (V_0, v_0) that leaves step N - 1 re-enters step 0.  One lap maps it affinely and
 * block-triangularly, y_out = Phi y + s_y, X_out = Phi X Phi' + L(y) + S_X with Phi the closed-loop monodromy, and the
 * fixed point takes three sweeps of the period -- A from (0, 0), B from (0, y*), C from (X*, y*), which writes the
 * gradients -- on one wave per (instance, segment) (`segments` clamped to N: len = ceil(N / segments), P = ceil(N / len)),
 * and two stitches on one wave per instance: y* = (I - Phi)^-1 s_y by pivoted elimination, and X* = Phi X* Phi' + W by Smith
 * doubling, X <- X + Phi_k X Phi_k', Phi_{k+1} = Phi_k^2, until max|Phi_k X Phi_k'| <= tol max(1, max|X|) and
 * max|Phi_{k+1}| <= 1e-3; max_iter 0 -> 40, tol 0 -> 4 DBL_EPSILON.  A finish ORs the status words and writes
 * residual[B] (optional): max(max|X_out - X*| / max(1, max|X*|), max|y_out - y*| / max(1, max|y*|)) for the adjoint that
 * leaves the last segment of pass C, a self-check; iterations[B] (optional): the Smith steps.
 * Stride-0 sums: a batch stride of 0 sums over the batch through per-instance records in the workspace and the
 * fixed-order two-stage sum of tfmpc_tvlqr_backward_vjp_f64 (chunks of 64, then a tree; no atomics); a requested output
 * with a time stride of 0 and N > 1 is summed in the sweep in time order, and the call then runs with ONE segment.
 * Checks, before any launch: B < 0, n, m, N <= 0: TFMPC_ERR_ARG; n > 32 or m > 32: TFMPC_ERR_UNSUPPORTED; segments < 1,
 * max_iter < 0, tol < 0 or NaN: TFMPC_ERR_ARG; B == 0 is a no-op; a NULL model operand, K, k, V, v, fwd_status or status,
 * a negative stride: TFMPC_ERR_ARG; more than INT32_MAX waves: TFMPC_ERR_UNSUPPORTED; a workspace that is NULL or too
 * small: TFMPC_ERR_WORKSPACE; not 8-byte aligned: TFMPC_ERR_ARG.  The workspace is always required.  In doubles, every
 * array rounded up to 64, with w = B P:
 *   3 up64(w n n) + 2 up64(w n) + up64(B n n)      Psi_s, W_s, X_s; s_s, y_s; Phi
 *   + for B > 1, sum over dF, df, dC, dc of up64(B N size) + up64(ceil(B / 64) N (n + m)^2)     the batch sum's records and
 *                                                     partial sums, size = n (n + m), n, (n + m)^2, n + m
 *   + up64(ceil((3 w + 2 B) / 2))                   the status words
 * times 8 bytes: what tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64 returns, enough for any choice of outputs and strides
 * (0 for an invalid or unsupported argument); a call needs only the records of the outputs it sums.
 * status[b]: the forward's word where fwd_status[b] is set; TFMPC_ST_NOT_PD for a non-positive Q_uu pivot;
 * TFMPC_ST_SINGULAR for a zero pivot in I - Phi; TFMPC_ST_NOT_STABILISING when the doubling meets a non-finite value or
 * does not stop within max_iter steps (a caller's own K may not be stabilising); TFMPC_ST_NAN for a non-finite y or
 * outgoing adjoint.  A phase does not run on an instance an earlier phase flagged.  A flagged instance has NaN in its own
 * gradient rows, in its residual and in every batch sum that contains it; no other instance is affected.  No atomics, no
 * allocation, no sync: an instance's bits depend on neither B nor its position, and repeated calls give identical bits.
 * kernel_name: "tvp_vjp_f64_wave16" (n <= 16 and m <= 16; 38.875 KiB of LDS in pass A) or "tvp_vjp_f64_wave32" (149.75
 * KiB, one wave per CU), "unsupported", "invalid".  TFMPC_TVLQR_TP_PHASES = 1 .. 5 stops the call after pass A / stitch A
 * / pass B / stitch B / pass C (TFMPC_TVLQR_TP_STOPPED; timing only). */
size_t tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(int B, int n, int m, int N, int segments);
const char *tfmpc_tvlqr_periodic_vjp_kernel_name_f64(int n, int m, int N, int segments);
int tfmpc_tvlqr_periodic_vjp_f64(int B, int n, int m, int N,
                                 const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                                 const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                                 const double *K, const double *k, const double *V, const double *v, const int32_t *fwd_status,
                                 const double *gK, const double *gk, const double *gV, const double *gv,
                                 double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                                 double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t,
                                 double *residual, int32_t *iterations, int32_t *status, int segments, int max_iter, double tol,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------- control-limited TV-LQR gradients --------
 * tfmpc_tvlqr_vjp_f32 at the optimum of the CONTROL-LIMITED problem, low <= u_t <= high.  low, high:
 * [m] per (b, t) with a batch and a time stride in elements (0 = shared), +-inf allowed.  Control i of instance b is HELD
 * at step t iff actions[b][t][i] equals low or high bit for bit (a forward that clips leaves the bound's bits on a
 * clamped control).  There is no multiplier test: a control on its bound with a zero multiplier counts as held, as in
 * Amos et al. 2018 (differentiable MPC).  Held controls have du = 0 in the adjoint: the adjoint solve runs on the model
 * with column n + i of F_t, row and column n + i of C_t (unit diagonal) and entry n + i of the linear term taken out AS
 * THE MODEL IS LOADED -- no masked copy exists; the workspace exceeds tfmpc_tvlqr_vjp_workspace_bytes by at most
 * B T (4 + 8 m) + 4096 bytes.  All other arguments, outputs, stride-0 sums, status and NaN rules as tfmpc_tvlqr_vjp_f32.
 * dlow, dhigh (optional): the gradient of the bound a held control sits on (low when it equals both), exactly 0 elsewhere,
 * each with its own batch and time stride (0 sums over that axis, fixed order, no atomics).  clamp_mask[B][T] (optional):
 * bit i = control i held at step t.  m <= 32; shapes as tfmpc_tvlqr_vjp_f32 otherwise (kernel_name: "unsupported"). */
size_t tfmpc_tvlqr_box_vjp_workspace_bytes(int B, int n, int m, int T);
const char *tfmpc_tvlqr_box_vjp_kernel_name(int n, int m, int T);
int tfmpc_tvlqr_box_vjp_f32(int B, int n, int m, int T,
                            const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                            const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                            const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                            const float *low, long slow_b, long slow_t, const float *high, long shigh_b, long shigh_t,
                            const float *states, const float *actions,
                            const float *g_states, const float *g_actions, const float *g_costs,
                            float *dF, long sdF_b, long sdF_t, float *df, long sdf_b, long sdf_t,
                            float *dC, long sdC_b, long sdC_t, float *dc, long sdc_b, long sdc_t,
                            float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b, float *dx0, long sdx0_b,
                            float *dlow, long sdlow_b, long sdlow_t, float *dhigh, long sdhigh_b, long sdhigh_t,
                            uint32_t *clamp_mask, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------- control-limited TV-LQR gradients, double precision --------
 * tfmpc_tvlqr_box_vjp_f32's contract with every value a double: the same argument list in the same
 * order, strides in ELEMENTS, the held set read off the actions' DOUBLE bits (low when a control equals both bounds, no
 * multiplier test), the same outputs, stride-0 sums in a fixed order without atomics, exact zeros in dlow / dhigh off the
 * held set and on the other bound, clamp_mask, B == 0 a no-op, the same checks in the same order before any launch.  The
 * costates are NOT that call's open-loop recursion but tfmpc_tvlqr_vjp_f64's value-function form on the REDUCED problem
 * (held controls fixed at their bounds): lam_t = V^m_t x_t + v^m_t, dlam_t = V^m_t dx_t + v~_t, with V^m, v~ from the
 * adjoint sweep on the masked model and v^m from a second masked backward sweep with the linear terms
 * f_t + F_t[:, n + H_t] u_H, c_t + C_t[:, n + H_t] u_H and the true final cost; no input beyond the f32 call's is needed.
 * status[B] (required) gets the OR of both sweeps' status words; an instance with any bit set has NaN in its own gradient
 * rows, dlow / dhigh included, and in every batch-summed gradient.  n <= 32 and m <= 32 (kernel_name:
 * "tv_masked_f64_wave16" for n <= 16 and m <= 16, "tv_masked_f64_wave32" otherwise; "unsupported" beyond, "invalid" for
 * n <= 0 or m <= 0), TFMPC_ERR_UNSUPPORTED beyond.  With up(x) = x rounded up to a multiple of 64, d = n + m and
 * chunks = ceil(B / 256), the workspace holds tfmpc_tvlqr_vjp_workspace_bytes_f64(B, n, m, T) plus
 *   8 * [ up(ceil(B T / 2)) + up(ceil(B / 2)) + 3 up(B T m) + 2 up(B T n) + up(B T d) ]  bytes
 * (held-set words, the second sweep's status, the unmasked g_u and the two bound records, f^ and v^m, c^); 0 for B <= 0.
 * The workspace must be 8-byte aligned (TFMPC_ERR_ARG otherwise, after the size check): doubles are carved from it. */
size_t tfmpc_tvlqr_box_vjp_workspace_bytes_f64(int B, int n, int m, int T);
const char *tfmpc_tvlqr_box_vjp_kernel_name_f64(int n, int m, int T);
int tfmpc_tvlqr_box_vjp_f64(int B, int n, int m, int T,
                            const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                            const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                            const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                            const double *low, long slow_b, long slow_t, const double *high, long shigh_b, long shigh_t,
                            const double *states, const double *actions,
                            const double *g_states, const double *g_actions, const double *g_costs,
                            double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                            double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t,
                            double *dCfin, long sdCfin_b, double *dcfin, long sdcfin_b, double *dx0, long sdx0_b,
                            double *dlow, long sdlow_b, long sdlow_t, double *dhigh, long sdhigh_b, long sdhigh_t,
                            uint32_t *clamp_mask, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------ control-limited TV-LQR, the solve --------
 * The forward of tfmpc_tvlqr_box_vjp_f32: the optimum of the TV-LQR problem under low <= u_t <= high.
 * Model operands, Cfin / cfin and their strides as in tfmpc_tvlqr_solve_f32; low, high as in tfmpc_tvlqr_box_vjp_f32
 * ([m] per (b, t), batch and time strides in elements, +-inf allowed; low <= high is a PRECONDITION).  u_init: [T][m] per
 * instance with batch stride su_b (0 = shared), NULL = zeros; it is clipped into the box.  The problem is a convex QP with
 * an exact model (PRECONDITION as the TV-LQR block: C_t symmetric, C_t >= 0, C_t,uu > 0), solved by control-limited Newton
 * sweeps without regularisation: per pass a backward sweep in delta form around the nominal with a projected-Newton box-QP
 * per step (warm start 0, at most 100 iterations: TFMPC_ST_QP_MAXITER; the free block eliminated without pivoting, a
 * non-positive pivot: TFMPC_ST_NOT_PD), then the first of the step sizes 1, 1/2, ..., 2^-10 whose clipped closed-loop
 * rollout lowers the total cost (taken untested, at most three passes in a row, while the predicted decrease is below
 * 1e-6 max(1, |J|), the rounding of J).  Stops when max |k_t,i| <= tol max(1, max |u|) (tol = 0: 4e-6), after max_iter
 * passes (0: 100; TFMPC_ST_MAX_ATTEMPTS), or when no step size lowers the cost.  The sweep that meets the stop rule still
 * has its step applied, in full and untested (a step of tol left out is several fp32 roundings of the optimum): the total
 * cost after this last step is NOT checked to have decreased, the step does not count towards the three trusted passes,
 * and clamp_mask holds the held sets of the sweep that produced it.  status reports the LAST sweep only: a
 * TFMPC_ST_QP_MAXITER raised in an earlier pass is dropped when a later pass runs.
 * Outputs: states[B][T+1][n], actions[B][T][m], costs[B][T+1] of the final nominal -- a control on a bound carries the
 * bound's bits, which is what tfmpc_tvlqr_box_vjp_f32's held-set rule reads; iterations[B], the backward sweeps run (0
 * when low == high everywhere); status[B]; reason[B] (optional): 0 converged by the step norm, 1 no step size lowered the
 * cost, 2 the pass cap, 3 flagged; clamp_mask[B][T] (optional): the last sweep's held sets, bit i = control i (zero for
 * an instance that ran no sweep).  An instance flagged TFMPC_ST_NOT_PD or
 * TFMPC_ST_NAN gets NaN in its own rows of states, actions and costs and touches nothing else; one flagged
 * TFMPC_ST_QP_MAXITER or TFMPC_ST_MAX_ATTEMPTS keeps its last feasible nominal.  One wave per instance, no horizon cap, no
 * atomics; m <= 32 and whatever one wave's LDS holds (n = m = 32 included), TFMPC_ERR_UNSUPPORTED beyond (kernel_name:
 * "unsupported").  workspace: tfmpc_tvlqr_box_solve_workspace_bytes(B, n, m, T) = 4 B (T m (n + 1) + (T + 1) n + T m + T + 1)
 * bytes (gains and the candidate trajectory).  Error codes before any launch: TFMPC_ERR_ARG (sizes, max_iter < 0, tol < 0
 * or NaN, NULL pointers, negative strides), TFMPC_ERR_UNSUPPORTED, TFMPC_ERR_WORKSPACE.  B == 0 is a no-op. */
size_t tfmpc_tvlqr_box_solve_workspace_bytes(int B, int n, int m, int T);
const char *tfmpc_tvlqr_box_solve_kernel_name(int n, int m, int T);
int tfmpc_tvlqr_box_solve_f32(int B, int n, int m, int T,
                              const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                              const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                              const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
                              const float *low, long slow_b, long slow_t, const float *high, long shigh_b, long shigh_t,
                              const float *x0, const float *u_init, long su_b, int max_iter, float tol,
                              float *states, float *actions, float *costs,
                              int32_t *iterations, int32_t *status, int32_t *reason, uint32_t *clamp_mask,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------ control-limited TV-LQR, the solve in double --------
 * tfmpc_tvlqr_box_solve_f32 in double precision: the same algorithm, loop caps, status / reason /
 * iterations / clamp_mask semantics and NaN rows, with every float a double (tol included; strides stay in ELEMENTS).
 * tol = 0 selects 1e-12; the trusted-step ratio stays 1e-6 and the Armijo constant 1e-4.  Products run on the f64 matrix
 * cores.  One wave per instance, n <= 32 and m <= 32 (kernel_name: "tv_box_f64_wave16" for n <= 16 and m <= 16,
 * "tv_box_f64_wave32" otherwise; "unsupported" beyond, "invalid" for n <= 0 or m <= 0), TFMPC_ERR_UNSUPPORTED beyond.
 * workspace: tfmpc_tvlqr_box_solve_workspace_bytes_f64(B, n, m, T) = 8 B (T m (n + 1) + (T + 1) n + T m + T + 1) bytes, 0
 * for B <= 0.  The same argument, shape and workspace checks in the same order; B == 0 is a no-op.  A control on a
 * bound carries the double bound's bits, which is what tfmpc_tvlqr_box_vjp_f64's held-set rule reads. */
size_t tfmpc_tvlqr_box_solve_workspace_bytes_f64(int B, int n, int m, int T);
const char *tfmpc_tvlqr_box_solve_kernel_name_f64(int n, int m, int T);
int tfmpc_tvlqr_box_solve_f64(int B, int n, int m, int T,
                              const double *F, long sF_b, long sF_t, const double *f, long sf_b, long sf_t,
                              const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                              const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                              const double *low, long slow_b, long slow_t, const double *high, long shigh_b, long shigh_t,
                              const double *x0, const double *u_init, long su_b, int max_iter, double tol,
                              double *states, double *actions, double *costs,
                              int32_t *iterations, int32_t *status, int32_t *reason, uint32_t *clamp_mask,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------- infinite-horizon LQR --------
 * The stationary solution of tfmpc_lqr_*_f32's problem: A = F[:, :n], B = F[:, n:], Q = C_xx,
 * S = C_xu, R = C_uu (C symmetric).  P is the stabilising solution of the discrete algebraic Riccati equation, found by
 * the structure-preserving doubling algorithm; then K = -(R + B'PB)^-1 (B'PA + S'), A_cl = A + BK,
 * p = (I - A_cl')^-1 (c_x + K'c_u + A_cl'Pf), k = -(R + B'PB)^-1 (c_u + B'(Pf + p)): the limits of the finite
 * recursion's K_t, k_t, V_t, v_t.  Outputs K[B][m][n], k[B][m], P[B][n][n], p[B][n] (each may be NULL),
 * iterations[B] (doubling steps taken, optional), status[B] (required).  Batch strides in elements, 0 = shared.
 * max_iter = 0 / tol = 0.0f select the defaults: 40 doubling steps, and a stop when max|H_{k+1} - H_k| <= tol max|H_{k+1}|
 * with tol = 4 FLT_EPSILON (and max|A_{k+1}| <= 1e-3).  status: TFMPC_ST_NOT_PD (R or R + B'PB not positive definite),
 * TFMPC_ST_SINGULAR (a zero pivot in I + GH or I - A_cl'), TFMPC_ST_NOT_STABILISING; a flagged instance gets NaN in its
 * own outputs, no other instance is affected.  n <= 16, m <= 16: one wave per instance, products on the f32 matrix cores;
 * n <= 32, m <= 32: the same algorithm with 32-wide LDS tiles; beyond: TFMPC_ERR_UNSUPPORTED.  B == 0 is a no-op. */
const char *tfmpc_lqr_steady_state_kernel_name(int n, int m);
int tfmpc_lqr_steady_state_f32(int B, int n, int m,
                               const float *F, long sF_b, const float *f, long sf_b,
                               const float *C, long sC_b, const float *c, long sc_b,
                               int max_iter, float tol,
                               float *K, float *k, float *P, float *p,
                               int32_t *iterations, int32_t *status, void *stream);

/* tfmpc_lqr_steady_state_f32 in double: the same algorithm, argument rules, status bits and NaN
 * outputs, every operand and output double, products on the f64 matrix cores.  tol = 0.0 selects 4 DBL_EPSILON.
 * n <= 16, m <= 16: "ss_f64_wave16"; n <= 32, m <= 32: "ss_f64_wave32" (116 KiB of dynamic LDS, one wave per CU);
 * beyond: TFMPC_ERR_UNSUPPORTED.  No workspace, no atomics. */
const char *tfmpc_lqr_steady_state_kernel_name_f64(int n, int m);
int tfmpc_lqr_steady_state_f64(int B, int n, int m,
                               const double *F, long sF_b, const double *f, long sf_b,
                               const double *C, long sC_b, const double *c, long sc_b,
                               int max_iter, double tol,
                               double *K, double *k, double *P, double *p,
                               int32_t *iterations, int32_t *status, void *stream);

/* Vector-Jacobian product of tfmpc_lqr_steady_state_f32: given the forward's K[B][m][n], k[B][m],
 * P[B][n][n], p[B][n] and status[B] (fwd_status), and upstream gradients gK, gk, gP, gp of the same per-instance layout
 * (each NULL = zero), writes the gradients of <gK, K> + <gk, k> + <gP, P> + <gp, p> with respect to F, f, C, c.  Model
 * operands and their batch strides as in the forward.  The explicit formulas of K, k, p are reversed with one
 * elimination of R + B'PB (without pivoting: TFMPC_ST_NOT_PD) and one of I - A_cl (pivoted: TFMPC_ST_SINGULAR); P's
 * dependence through the Riccati equation is one Stein solve Y = A_cl Y A_cl' + sym(Pbar) by Smith doubling, stopped
 * when max|Phi Y Phi'| <= tol max|Y| and max|Phi^2| <= 1e-3 (max_iter = 0 / tol = 0.0f: 40 steps, 4 FLT_EPSILON),
 * else TFMPC_ST_NOT_STABILISING.  Outputs dF[B][n][n+m], df[B][n], dC[B][d][d] (the symmetric gradient), dc[B][d], each
 * with its own batch stride in elements; a NULL output is not computed, a stride of 0 SUMS the gradient over the batch
 * (fixed-order reduction without atomics: repeated calls give identical bits).  status[B] (required) gets the forward's
 * status where it was flagged, else the backward's; a flagged instance has NaN in its own gradient rows and in every
 * batch-summed gradient.  workspace: tfmpc_lqr_steady_state_vjp_workspace_bytes(B, n, m) bytes serve any choice of
 * summed outputs (NULL is fine when no output is summed).  Shapes as the forward serves; B == 0 is a no-op. */
size_t tfmpc_lqr_steady_state_vjp_workspace_bytes(int B, int n, int m);
const char *tfmpc_lqr_steady_state_vjp_kernel_name(int n, int m);
int tfmpc_lqr_steady_state_vjp_f32(int B, int n, int m,
                                   const float *F, long sF_b, const float *f, long sf_b,
                                   const float *C, long sC_b, const float *c, long sc_b,
                                   const float *K, const float *k, const float *P, const float *p, const int32_t *fwd_status,
                                   const float *gK, const float *gk, const float *gP, const float *gp,
                                   int max_iter, float tol,
                                   float *dF, long sdF_b, float *df, long sdf_b, float *dC, long sdC_b, float *dc, long sdc_b,
                                   int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* tfmpc_lqr_steady_state_vjp_f32 in double, for the K, k, P, p of tfmpc_lqr_steady_state_f64: the
 * same sequence, argument rules, status bits and NaN rows, every operand, upstream gradient and output double,
 * products on the f64 matrix cores, the batch sums in the same fixed order with double accumulators.  tol = 0.0 selects
 * 4 DBL_EPSILON.  n <= 16, m <= 16: "ss_vjp_f64_wave16"; n <= 32, m <= 32: "ss_vjp_f64_wave32" (118 KiB of dynamic LDS,
 * one wave per CU); beyond: TFMPC_ERR_UNSUPPORTED.  workspace: tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(B, n, m)
 * bytes (the fp32 plan's element counts, 8 bytes each). */
size_t tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(int B, int n, int m);
const char *tfmpc_lqr_steady_state_vjp_kernel_name_f64(int n, int m);
int tfmpc_lqr_steady_state_vjp_f64(int B, int n, int m,
                                   const double *F, long sF_b, const double *f, long sf_b,
                                   const double *C, long sC_b, const double *c, long sc_b,
                                   const double *K, const double *k, const double *P, const double *p, const int32_t *fwd_status,
                                   const double *gK, const double *gk, const double *gP, const double *gp,
                                   int max_iter, double tol,
                                   double *dF, long sdF_b, double *df, long sdf_b, double *dC, long sdC_b, double *dc, long sdc_b,
                                   int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* --------------------------------------------------------------- iLQR --------
 * Control-limited iLQR (tfmpc/solvers/ilqr.py) over the reference's differentiable
 * environments (tfmpc/envs).  An environment is described by a kind tag plus
 * parameter arrays; Jacobians / Hessians are closed forms evaluated on the device
 * (the reference obtains them by autodiff, tfmpc/envs/diffenv.py:13-101).
 */
#define TFMPC_ENV_LQ 0          /* (F, f, C, c) of tfmpc/solvers/lqr.py:36-57 as an env: n != m allowed */
#define TFMPC_ENV_NAVLQR 1      /* tfmpc/envs/lqr/navigation/__init__.py:8-47                           */
#define TFMPC_ENV_NAVIGATION 2  /* tfmpc/envs/navigation/__init__.py:9-74  (cec=True)                   */
#define TFMPC_ENV_HVAC 3        /* tfmpc/envs/hvac/__init__.py:8-149                                    */
#define TFMPC_ENV_RESERVOIR 4   /* tfmpc/envs/reservoir/__init__.py:9-105 (cec=True)                    */
#define TFMPC_ENV_USER 5        /* ANY differentiable env (tfmpc/envs/diffenv.py:13-101 differentiates whatever it is handed): transition /
                                   cost / final_cost given as device functions, derivatives by forward-mode dual numbers in the kernel.  Not
                                   served by this library's entry points (TFMPC_ERR_ARG): tfmpc.envs.deviceenv compiles csrc/user_env_kernels.hip.in
                                   around the user's source into a companion library that exports tfmpc_userenv_* twins of the env-dependent
                                   entry points (rollout, derivatives, forward, solve_trace; same signatures).  p0 = the env's parameter
                                   floats, n_zones of them per instance. */
#define TFMPC_ENV_MAX_PARAMS 10
#define TFMPC_MAX_ALPHAS 16

/* Parameter arrays p[i] per kind (device pointers, fp32; stride[i] = element
 * distance between instances, 0 = shared by the whole batch):
 *   LQ         p0 F[n][n+m]  p1 f[n]  p2 C[n+m][n+m]  p3 c[n+m]
 *   NAVLQR     p0 goal[n]; scalar[0] = beta
 *   NAVIGATION p0 goal[n]  p1 center[Z][n]  p2 decay[Z]           (n_zones = Z, n <= 8)
 *   HVAC       p0 temp_outside  p1 temp_hall  p2 temp_lower_bound  p3 temp_upper_bound
 *              p4 adj_outside/R_outside  p5 adj_hall/R_hall  p6 capacity  p7 air_max   (all [n])
 *              p8 G[n][n] = (adj | adj^T) / R_wall
 *   RESERVOIR  p0 max_res_cap  p1 lower_bound  p2 upper_bound  p3 low_penalty  p4 high_penalty
 *              p5 set_point_penalty  p6 rain_shape*rain_scale   (all [n])  p7 downstream[n][n]
 * low[m] / high[m]: action bounds (+-inf allowed, shared by the batch); `bounded`
 * is gym's Box.is_bounded(): every bound finite (ilqr.py:136). */
typedef struct TfmpcEnv {
    int32_t kind, n, m, n_zones, bounded;
    int32_t any_finite_bound;   /* 1 if any entry of low/high is finite (forward clips, ilqr.py:197) */
    int32_t coupling_shift;     /* RESERVOIR only, a PROMISE by the caller: +1 = `downstream` is the chain i -> i + 1 (D[i][i+1] = 1, every other
                                   entry 0), -1 = the chain i -> i - 1, 0 = no statement (any matrix).  Every config the reference holds
                                   is a chain (tests/conftest.py:70-75, reservoir/res4.config.json:13-18); with the promise a large batch runs an
                                   instantiation without coupling products.  Checked on the device against p7 before anything is computed:
                                   a broken promise leaves TFMPC_ST_ENV_FLAG in status[b] and the outputs untouched.  (Row moves
                                   equal the products for FINITE states; a product spreads one row's Inf / NaN into every row, a row move
                                   hands it to the neighbour only: a DIVERGING instance's status can differ from TFMPC_COSTATE_COUPLING=dense.) */
    int32_t reserved2;
    const float *low, *high;
    const float *p[TFMPC_ENV_MAX_PARAMS];
    int64_t stride[TFMPC_ENV_MAX_PARAMS];
    float scalar[4];
} TfmpcEnv;

/* Solver hyper-parameters (ilqr.py:27-37) + the line-search step sizes
 * np.geomspace(1, alpha_min, 11) (ilqr.py:322) computed by the host. */
typedef struct TfmpcIlqrConfig {
    float atol;             /* 5e-3 */
    int32_t max_iterations; /* 100  */
    float mu_min;           /* 1e-6 */
    float delta_0;          /* 2.0  */
    float c1;               /* 0.0  */
    int32_t n_alphas;       /* 11   */
    float alphas[TFMPC_MAX_ALPHAS];
    int32_t max_attempts;   /* cap on rejected backward/line-search attempts per solve (the
                               reference loops without bound, ilqr.py:238-270) */
    int32_t storage_bf16;   /* 1: trajectories (and gains) kept in HBM between passes are rounded to bf16 when
                               stored, arithmetic stays fp32 -- BASELINE configs[4] "fp32 vs bf16".  HVAC /
                               Reservoir envs shared by the batch: REAL 16-bit containers in the workspace (half
                               the bytes); other envs: the wave kernel emulates the format in fp32 containers.
                               Outputs are fp32 arrays holding bf16-representable values either way. */
} TfmpcIlqrConfig;

/* iLQR.start (ilqr.py:53-82) with the random actions injected: roll the env from
 * x0[B][n] under actions[B][T][m]; writes states[B][T+1][n], costs[B][T+1]. */
int tfmpc_ilqr_rollout_f32(const TfmpcEnv *env, int B, int T, const float *x0, const float *actions,
                           float *states, float *costs, void *stream);

/* iLQR.derivatives (ilqr.py:84-92) = DiffEnv.get_linear_transition / get_quadratic_cost /
 * get_quadratic_final_cost (diffenv.py:13-101) at every (x_t, u_t), t < T, and at x_T.
 * states[B][T+1][n], actions[B][T][m].  Outputs (any may be NULL): f[B][T][n],
 * f_x[B][T][n][n], f_u[B][T][n][m], l[B][T], l_x[B][T][n], l_u[B][T][m], l_xx[B][T][n][n],
 * l_uu[B][T][m][m], l_ux[B][T][m][n], l_xu[B][T][n][m]; final fl[B], fl_x[B][n], fl_xx[B][n][n]. */
int tfmpc_ilqr_derivatives_f32(const TfmpcEnv *env, int B, int T, const float *states, const float *actions,
                               float *f, float *f_x, float *f_u, float *l, float *l_x, float *l_u,
                               float *l_xx, float *l_uu, float *l_ux, float *l_xu,
                               float *fl, float *fl_x, float *fl_xx, void *stream);

/* iLQR.backward (ilqr.py:94-172) on materialised models (layouts as above).  mu[B]
 * (mu_stride 1) or one shared value (mu_stride 0).  Controller per step: Cholesky-type
 * solve (:357-362), box-QP (:364-387 + tfmpc/utils/optimization.py:6-101) when `bounded`
 * and V_xx != 0, bang-bang otherwise (:140-141).  Outputs K[B][T][m][n], k[B][T][m], J[B],
 * dV1[B], dV2[B]; status[B] gets TFMPC_ST_NOT_PD where the reference would raise
 * InvalidArgumentError (outputs of that instance are then undefined). */
int tfmpc_ilqr_backward_f32(int B, int n, int m, int T, const float *actions,
                            const float *f_x, const float *f_u, const float *l, const float *l_x,
                            const float *l_u, const float *l_xx, const float *l_uu, const float *l_xu,
                            const float *fl, const float *fl_x, const float *fl_xx,
                            const float *low, const float *high, int bounded,
                            const float *mu, long mu_stride,
                            float *K, float *k, float *J, float *dV1, float *dV2, int32_t *status, void *stream);

/* iLQR.forward (ilqr.py:174-212): closed-loop rollout around (x[B][T+1][n], u[B][T][m])
 * with gains K, k and step alpha[B] (alpha_stride 1) or shared (0).  Outputs states,
 * actions, costs[B][T+1], J[B], residual[B]. */
int tfmpc_ilqr_forward_f32(const TfmpcEnv *env, int B, int T, const float *x, const float *u,
                           const float *K, const float *k, const float *alpha, long alpha_stride,
                           float *states, float *actions, float *costs, float *J, float *residual,
                           void *stream);

/* Scratch of tfmpc_ilqr_solve_f32, a function of the shape alone (the env kind is not known here): per instance the
 * gains K, k and one candidate trajectory; for n = m = 2 a line-search block per wavefront; for n = m <= 32 the two
 * wave-major trajectory buffers of the 16-instances-per-wave HVAC / Reservoir kernel (+ for n <= 16 the coefficients
 * of its two-part costate sweep: 3 KB per group and time step).  The control-limited LQ kernel keeps its helper teams'
 * board (TFMPC_BOX_HELPERS: ~60 KB per team) in the candidate-trajectory part: no extra bytes.  The workspace handed to
 * tfmpc_ilqr_solve_f32 must be 256-byte aligned (TFMPC_ERR_WORKSPACE otherwise). */
size_t tfmpc_ilqr_workspace_bytes(int B, int n, int m, int T);
/* The same for ONE env (round 6): only the parts the kernels of that env kind read -- never more than tfmpc_ilqr_workspace_bytes of its shape, and
 * hundreds of MB less at large batches (an HVAC / Reservoir batch does not carry the LQ kernels' slab, an LQ batch not the costate kernel's buffers,
 * neither the 2-D envs' scratch).  tfmpc_ilqr_solve*_f32 accept either size.  0 for a null env or a bad shape. */
size_t tfmpc_ilqr_workspace_bytes_for(const TfmpcEnv *env, int B, int T);

/* iLQR.solve (ilqr.py:214-283) in ONE launch: each wave runs its instance's whole
 * iteration loop (linearise on the fly, regularised backward pass with the local
 * Cholesky-failure retry of :285-315, 11-point line search :317-355, mu/delta schedule
 * :259-270, both convergence tests :243-257).  u_init[B][T][m] are the start actions
 * (ilqr.py:70 draws them from TF's RNG; the host injects them).  Outputs: the final
 * nominal trajectory states[B][T+1][n], actions[B][T][m], costs[B][T+1];
 * iterations[B] = the reference's returned loop index; status[B]. */
int tfmpc_ilqr_solve_f32(const TfmpcEnv *env, const TfmpcIlqrConfig *cfg, int B, int T,
                         const float *x0, const float *u_init,
                         float *states, float *actions, float *costs,
                         int32_t *iterations, int32_t *status,
                         void *workspace, size_t workspace_bytes, void *stream);

/* tfmpc_ilqr_solve_f32 with the DECISION TRACE of the solve (what the reference prints per pass through the body of
 * ilqr.py:238-270 -- `[BACKWARD] J_hat`, `[SOLVE] g_norm`, `[FORWARD] J`, the progress bar's J / g_norm / residual,
 * ilqr.py:243-279 -- and what its regularisation schedule holds): one row of TFMPC_TRACE_COLS floats per backward
 * pass + line search of an instance, in the order they happen, trace[B][trace_rows][TFMPC_TRACE_COLS]; rows beyond
 * trace_rows are dropped.  trace_len[B] = the number of passes the instance made (may exceed trace_rows).
 * Columns: see TFMPC_TR_*.  trace == NULL: identical to tfmpc_ilqr_solve_f32.  With a trace the solve runs on a
 * kernel that records one (the HVAC / Reservoir shared-env kernel, the 2-D lane-group kernel, else the generic
 * wave kernel): same algorithm, possibly another kernel than the untraced call would pick. */
#define TFMPC_TRACE_COLS 11
#define TFMPC_TR_ITERATION 0  /* the reference's loop index `iteration` (ilqr.py:227) of this pass            */
#define TFMPC_TR_MU 1         /* mu handed to _backward (ilqr.py:240), before a local Cholesky-failure bump   */
#define TFMPC_TR_DELTA 2      /* delta at that point                                                          */
#define TFMPC_TR_J_HAT 3      /* cost of the nominal trajectory as the backward pass sums it (ilqr.py:164)    */
#define TFMPC_TR_G_NORM 4     /* ilqr.py:243                                                                  */
#define TFMPC_TR_ALPHA_INDEX 5 /* position (0-based) in the step-size list of the LAST rollout of the line search;
                                 -1 when the pass ended on g_norm < atol before any rollout                  */
#define TFMPC_TR_ALPHA 6      /* that step size                                                               */
#define TFMPC_TR_J 7          /* its total cost J (ilqr.py:205-210)                                           */
#define TFMPC_TR_ACCEPTED 8   /* 1 = z >= c1 (ilqr.py:351-353), 0 = all step sizes rejected, -1 = no line search */
#define TFMPC_TR_RESIDUAL 9   /* ilqr.py:206 of that rollout (-1 without line search)                         */
#define TFMPC_TR_LEVEL 10     /* local regularisation bumps _backward needed before the pass factorised
                                 (ilqr.py:305-309; 0 = at TFMPC_TR_MU itself): the level whose gains the pass used */
int tfmpc_ilqr_solve_trace_f32(const TfmpcEnv *env, const TfmpcIlqrConfig *cfg, int B, int T,
                               const float *x0, const float *u_init,
                               float *states, float *actions, float *costs,
                               int32_t *iterations, int32_t *status,
                               float *trace, int trace_rows, int32_t *trace_len,
                               void *workspace, size_t workspace_bytes, void *stream);

/* tfmpc_ilqr_solve_trace_f32 that ALSO exports what the box-QP of every backward step ended on (version >= 300; test and
 * diagnosis instrument: ilqr.py:364-385 computes K_t from the free set optimization.py:35-72 returns, so two fp32 programs that
 * end a QP on different free sets differ DISCRETELY -- other rows of K_t are zero -- and no tolerance on numbers can compare them):
 * clamp_mask[B][trace_rows][T], bit a of entry (b, pass, t) set = action a was CLAMPED in the last factorised free set of that
 * step's QP (row a of K_t is zero); qp_iterations[B][trace_rows][T] = iterations of the projected-Newton loop
 * (optimization.py:24; 0 = the step ran no QP).  Both NULL: identical to tfmpc_ilqr_solve_trace_f32; both need `trace`.
 * Written by the control-limited matrix-core kernel (LQ env, n <= 16, m <= 8, bounded actions); other kernels leave the two
 * buffers untouched -- pre-fill them with 0xFF to tell. */
int tfmpc_ilqr_solve_trace_qp_f32(const TfmpcEnv *env, const TfmpcIlqrConfig *cfg, int B, int T,
                                  const float *x0, const float *u_init,
                                  float *states, float *actions, float *costs,
                                  int32_t *iterations, int32_t *status,
                                  float *trace, int trace_rows, int32_t *trace_len,
                                  uint8_t *clamp_mask, uint8_t *qp_iterations,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* projected_newton_qp (tfmpc/utils/optimization.py:6-101): B independent box QPs
 * min 1/2 x^T H x + q^T x, low <= x <= high.  H[B][m][m], q/low/high/x0[B][m];
 * outputs x[B][m], free[B][m] (1.0 / 0.0), status[B]. */
int tfmpc_boxqp_f32(int B, int m, const float *H, const float *q, const float *low, const float *high,
                    const float *x0, float *x, float *free_mask, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TFMPC_HIP_H */
