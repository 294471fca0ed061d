// tvlqr_box_body.h -- the STATEMENTS of the control-limited time-varying LQR forward solve, the one
// body of tvlqr_box_wave.h's kernels.  Included INSIDE the braces of a __global__ function, once per kernel, with in scope
//   P     the policy (tvlqr_box_wave.h),
//   p     the kernel's argument, a TvBoxArgsT<P::T>,
//   smem  the wave's dynamic LDS, a P::T *.
// It is text and not a device function on purpose: a __forceinline__ function around these statements compiles the
// fp32 kernel to other instructions than the statements written in the kernel itself (10 490 and 10 590 lines for a
// by-reference and a by-value argument against 10 169), and tvlqr_box.hip must keep its one non-template kernel.
// No include guard: every kernel includes it again.
    using S = typename P::T;
    const TvLqrArgsT<S> &a = p.a;
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m, T = a.T;
    TvSmem<S> s = tv_carve<false>(smem, n, m);
    const int ldd = s.ldd, ldn = s.ldn, lda = s.lda, ldv = s.ldv;
    const bool own = lane < m;                                   // lane r owns control r (m <= 32)
    const uint32_t all_held = m == 32 ? 0xFFFFFFFFu : ((1u << m) - 1u);

    const S *Cf = a.Cfin ? a.Cfin + (size_t)b * a.sCfin_b : tv_at(a.C, a.sC_b, a.sC_t, b, T - 1);
    const S *cf = a.Cfin ? a.cfin + (size_t)b * a.scfin_b : tv_at(a.c, a.sc_b, a.sc_t, b, T - 1);
    const int ldf = a.Cfin ? n : d;

    const size_t nx = ((size_t)T + 1) * n, nu = (size_t)T * m, nc = (size_t)T + 1;   // one instance's trajectory
    S *xs = a.states + b * nx;
    S *us = a.actions + b * nu;
    S *cs = a.costs + b * nc;
    S *cx = p.cx + b * nx;
    S *cu = p.cu + b * nu;
    S *cc = p.cc + b * nc;
    S *Kg = a.K + (size_t)b * a.sK;
    S *kg = a.k + (size_t)b * a.sk;
    uint32_t *maskg = p.clamp_mask ? p.clamp_mask + (size_t)b * T : nullptr;

    auto load_model = [&](int t, bool with_f) {
        load_matrix(s.F, ldd, tv_at(a.F, a.sF_b, a.sF_t, b, t), n, d);
        load_matrix(s.C, ldd, tv_at(a.C, a.sC_b, a.sC_t, b, t), d, d);
        const S *cg = tv_at(a.c, a.sc_b, a.sc_t, b, t);
        for (int i = lane; i < d; i += kWave) s.c[i] = cg[i];
        if (with_f) {
            const S *fg = tv_at(a.f, a.sf_b, a.sf_t, b, t);
            for (int i = lane; i < n; i += kWave) s.f[i] = fg[i];
        }
    };

    // A rollout from x0 into (ox, ou, oc); returns the total cost, summed in time order.
    //   INIT : u_t = clip(u_init_t or 0); any_free becomes true iff some low != high.
    //   else : u_t = clip(nominal u_t + alpha k_t + K_t (x_t - nominal x_t)) with the gains of the last sweep.
    bool any_free = false;
    auto rollout = [&](const S alpha, const bool init, S *ox, S *ou, S *oc) -> S {
        for (int i = lane; i < n; i += kWave) {
            const S x = a.x0[(size_t)b * n + i];
            s.z[i] = x;
            ox[i] = x;
        }
        S J = S(0);
        int loose = 0;
        for (int t = 0; t < T; ++t) {
            load_model(t, true);
            if (!init) {
                load_matrix(s.K, ldn, Kg + (size_t)t * m * n, m, n);
                for (int r = lane; r < m; r += kWave) s.k[r] = kg[(size_t)t * m + r];
                for (int i = lane; i < n; i += kWave) s.q[i] = s.z[i] - xs[(size_t)t * n + i];
            }
            wsync();
            if (own) {
                const S lo = tv_at(p.low, p.slow_b, p.slow_t, b, t)[lane];
                const S hi = tv_at(p.high, p.shigh_b, p.shigh_t, b, t)[lane];
                S u;
                if (init) {
                    u = p.u_init ? p.u_init[(size_t)b * p.su_b + (size_t)t * m + lane] : S(0);
                    loose |= lo != hi;
                } else {
                    S fb = S(0);
                    for (int j = 0; j < n; ++j) fb = fma(s.K[lane * ldn + j], s.q[j], fb);
                    u = fma(alpha, s.k[lane], us[(size_t)t * m + lane]) + fb;
                }
                u = fmin(fmax(u, lo), hi);
                s.z[n + lane] = u;
                ou[(size_t)t * m + lane] = u;
            }
            wsync();
            S part = S(0);                                     // 1/2 z^T C_t z + c_t^T z
            for (int r = lane; r < d; r += kWave) {
                S cz = S(0);
                for (int j = 0; j < d; ++j) cz = fma(s.C[r * ldd + j], s.z[j], cz);
                part += s.z[r] * (S(0.5) * cz + s.c[r]);
            }
            for (int i = lane; i < n; i += kWave) {            // x' = F_t z + f_t
                S x = s.f[i];
                for (int j = 0; j < d; ++j) x = fma(s.F[i * ldd + j], s.z[j], x);
                s.xn[i] = x;
            }
            const S cost = wave_sum(part);
            if (lane == 0) oc[t] = cost;
            if (init && maskg && lane == 0) maskg[t] = 0u;
            J += cost;
            wsync();
            for (int i = lane; i < n; i += kWave) {
                const S x = s.xn[i];
                s.z[i] = x;
                ox[(size_t)(t + 1) * n + i] = x;
            }
            wsync();
        }
        S part = S(0);                                         // 1/2 x^T C_fin x + c_fin^T x
        for (int r = lane; r < n; r += kWave) {
            S cz = S(0);
            for (int j = 0; j < n; ++j) cz = fma(Cf[r * ldf + j], s.z[j], cz);
            part += s.z[r] * (S(0.5) * cz + cf[r]);
        }
        const S last = wave_sum(part);
        if (lane == 0) oc[T] = last;
        if (init) any_free = __ballot(loose != 0) != 0;
        return J + last;
    };

    // One backward sweep around the nominal in (xs, us): gains into (Kg, kg), the held sets into maskg.  Returns the
    // sweep's status bits; kmax = max |k|, umax = max |u|, dV = sum k^T q_u + 1/2 k^T Q_uu k.
    auto sweep = [&](S &kmax, S &umax, S &dV) -> int {
        int st = 0;
        S kpart = S(0), upart = S(0);
        dV = S(0);
        kmax = umax = S(0);
        wave_for_2d(n, n, [&](int i, int j, int) { s.V[i * ldn + j] = Cf[i * ldf + j]; });
        for (int i = lane; i < n; i += kWave) {                 // v = C_fin x_T + c_fin
            S x = cf[i];
            for (int j = 0; j < n; ++j) x = fma(Cf[i * ldf + j], xs[(size_t)T * n + j], x);
            s.v[i] = x;
        }
        wsync();
        for (int t = T - 1; t >= 0; --t) {
            load_model(t, false);
            for (int i = lane; i < n; i += kWave) s.z[i] = xs[(size_t)t * n + i];
            if (own) s.z[n + lane] = us[(size_t)t * m + lane];
            wsync();
            // W = F_t^T V  [d][n]
            P::matmul(d, n, n,
                      [&](int r, int k) { return s.F[k * ldd + r]; },
                      [&](int k, int j) { return s.V[k * ldn + j]; },
                      [](int, int) { return S(0); },
                      [&](int r, int j, S x) { s.W[r * ldn + j] = x; });
            wsync();
            // Q = C_t + W F_t ; q = C_t z_t + c_t + F_t^T v
            P::matmul(d, d, n,
                      [&](int r, int k) { return s.W[r * ldn + k]; },
                      [&](int k, int j) { return s.F[k * ldd + j]; },
                      [&](int r, int j) { return s.C[r * ldd + j]; },
                      [&](int r, int j, S x) { s.Q[r * ldd + j] = x; });
            for (int r = lane; r < d; r += kWave) {
                S s1 = S(0), s2 = S(0);
                for (int j = 0; j < d; ++j) s1 = fma(s.C[r * ldd + j], s.z[j], s1);
                for (int k = 0; k < n; ++k) s2 = fma(s.F[k * ldd + r], s.v[k], s2);
                s.q[r] = s.c[r] + s1 + s2;
            }
            wsync();

            // ---- box-QP: min 1/2 x^T Q_uu x + q_u^T x, lo <= x <= hi, from x = 0 (projected Newton) ----
            const S *Quu = s.Q + n * ldd + n;
            S *xv = s.k, *gv = s.prow, *dv = s.z + n;           // x, gradient and trial move, shared through LDS
            const S ub = own ? s.z[n + lane] : S(0);
            const S lo = own ? tv_at(p.low, p.slow_b, p.slow_t, b, t)[lane] - ub : S(0);
            const S hi = own ? tv_at(p.high, p.shigh_b, p.shigh_t, b, t)[lane] - ub : S(0);
            upart = fmax(upart, wave_abs(ub));
            S x = S(0);
            uint32_t held = 0, prev = 0;
            bool full = false;
            int qp = TFMPC_ST_QP_MAXITER;
            wsync();                                            // ub is read before dv (over z_u) is written
            if (own) xv[lane] = S(0);
            wsync();
            for (int it = 0; it < kQpIterations; ++it) {
                S g = S(0);
                if (own) {
                    g = s.q[n + lane];
                    for (int j = 0; j < m; ++j) g = fma(Quu[lane * ldd + j], xv[j], g);
                    gv[lane] = g;
                }
                const bool cl = own && ((x <= lo && g > S(0)) || (x >= hi && g < S(0)));
                held = (uint32_t)__ballot(cl);
                if (it > 0 && held == prev && full) { qp = 0; break; }   // a full Newton step on this very set: aug is current
                wsync();
                wave_for_2d(m, s.width, [&](int r, int j, int) {
                    const bool fr = !(held >> r & 1u);
                    S v;
                    if (j < m) v = (fr && !(held >> j & 1u)) ? Quu[r * ldd + j] : (r == j ? S(1) : S(0));
                    else if (j == m) v = fr ? gv[r] : S(0);
                    else v = fr ? s.Q[(n + r) * ldd + (j - m - 1)] : S(0);
                    s.aug[r * lda + j] = v;
                });
                wsync();
                if (wave_gauss_jordan<false>(s.aug, lda, m, s.width, s.fac, s.prow)) { st |= TFMPC_ST_NOT_PD; qp = 0; break; }
                if (held == all_held) { qp = 0; break; }
                const S step = (own && !cl) ? -s.aug[lane * lda + m] : S(0);
                // Armijo backtracking along the projection arc; the decrease is g.d + 1/2 d^T Q_uu d (no cancellation)
                S alpha = S(1), xc = x;
                bool accepted = false;
                for (int bt = 0; bt < kQpBacktracks; ++bt) {
                    xc = fmin(fmax(fma(alpha, step, x), lo), hi);
                    const S dd = xc - x;
                    wsync();
                    if (own) dv[lane] = dd;
                    wsync();
                    S qd = S(0);
                    if (own)
                        for (int j = 0; j < m; ++j) qd = fma(Quu[lane * ldd + j], dv[j], qd);
                    const S gd = wave_sum(own ? g * dd : S(0));
                    const S df = gd + wave_sum(own ? S(0.5) * dd * qd : S(0));
                    if (df < S(0) && df <= P::kArmijo * gd) { accepted = true; break; }
                    alpha *= S(0.5);
                }
                if (!accepted) { qp = 0; break; }               // the rounding floor: x stays, aug belongs to `held`
                full = alpha == S(1) && __ballot(own && xc != x + step) == 0;
                x = xc;
                prev = held;
                wsync();
                if (own) xv[lane] = x;
                wsync();
            }
            st |= qp;
            if (st & TFMPC_ST_NOT_PD) return st;

            // gains: rows of held controls exactly 0, K_f = -Q_uu,ff^-1 Q_ux,f ; k = x
            wave_for_2d(m, n, [&](int r, int j, int idx) {
                const S v = (held >> r & 1u) ? S(0) : -s.aug[r * lda + m + 1 + j];
                s.K[r * ldn + j] = v;
                Kg[(size_t)t * m * n + idx] = v;
            });
            if (own) {
                kg[(size_t)t * m + lane] = x;
                kpart = fmax(kpart, wave_abs(x));
            }
            if (maskg && lane == 0) maskg[t] = held;
            wsync();
            // V' = Q_xx + Q_xu K ; v' = q_x + Q_xu k (Schur forms: K_c = 0 and (Q_uu k + q_u)_f = 0 at the QP's optimum)
            P::matmul(n, n, m,
                      [&](int i, int k) { return s.Q[i * ldd + n + k]; },
                      [&](int k, int j) { return s.K[k * ldn + j]; },
                      [&](int i, int j) { return s.Q[i * ldd + j]; },
                      [&](int i, int j, S v) { s.Vn[i * ldv + j] = v; });
            for (int i = lane; i < n; i += kWave) {
                S s1 = S(0);
                for (int k = 0; k < m; ++k) s1 = fma(s.Q[i * ldd + n + k], xv[k], s1);
                s.vn[i] = s.q[i] + s1;
            }
            S part = S(0);
            if (own) {
                S quk = S(0);
                for (int k = 0; k < m; ++k) quk = fma(Quu[lane * ldd + k], xv[k], quk);
                part = x * (S(0.5) * quk + s.q[n + lane]);
            }
            dV += wave_sum(part);
            wsync();
            wave_for_2d(n, n, [&](int i, int j, int) { s.V[i * ldn + j] = S(0.5) * (s.Vn[i * ldv + j] + s.Vn[j * ldv + i]); });
            for (int i = lane; i < n; i += kWave) s.v[i] = s.vn[i];
            wsync();
        }
        // (|k| may be NaN only with a NaN dV, which the caller tests; fmax drops it here)
        kmax = wave_max(kpart);
        umax = wave_max(upart);
        return st;
    };

    // The candidate becomes the nominal.
    auto adopt = [&]() {
        wsync();                                                // the candidate is visible to every lane
        for (size_t i = lane; i < nx; i += kWave) xs[i] = cx[i];
        for (size_t i = lane; i < nu; i += kWave) us[i] = cu[i];
        for (size_t i = lane; i < nc; i += kWave) cs[i] = cc[i];
        wsync();
    };

    const int max_iter = p.max_iter > 0 ? p.max_iter : kDefaultPasses;
    const S tol = p.tol > S(0) ? p.tol : P::kDefaultTol;
    int status = 0, reason = kReasonConverged, sweeps = 0, trusted = 0;

    S J = rollout(S(0), true, xs, us, cs);
    wsync();                                                    // the nominal is visible to every lane
    if (!(J == J)) status |= TFMPC_ST_NAN;
    if (any_free && !status) {
        reason = kReasonPassCap;
        for (int pass = 0; pass < max_iter; ++pass) {
            S kmax, umax, dV;
            status = sweep(kmax, umax, dV);                     // the last sweep's bits: an earlier pass's are dropped
            ++sweeps;
            if (!(dV == dV)) status |= TFMPC_ST_NAN;
            if (status & (TFMPC_ST_NOT_PD | TFMPC_ST_NAN)) { reason = kReasonFailed; break; }
            wsync();                                            // the gains are visible to every lane
            if (kmax <= tol * fmax(S(1), umax)) {
                // converged: the step is below tol but not below rounding, so it is applied in full, untested
                reason = kReasonConverged;
                if (kmax > S(0)) {
                    J = rollout(S(1), false, cx, cu, cc);
                    adopt();
                    if (!(J == J)) { status |= TFMPC_ST_NAN; reason = kReasonFailed; }
                }
                break;
            }
            // a predicted decrease below the rounding of J: J cannot rank candidates, the full step is taken untested
            const bool trust = -dV <= P::kTrustRatio * fmax(S(1), wave_abs(J)) && trusted < kTrustedInARow;
            trusted = trust ? trusted + 1 : 0;
            S alpha = S(1), Jn = J;
            bool accepted = false;
            for (int ls = 0; ls < kAlphas; ++ls) {
                Jn = rollout(alpha, false, cx, cu, cc);
                if (trust || Jn < J) { accepted = true; break; }
                alpha *= S(0.5);
            }
            if (!accepted) { reason = kReasonNoDecrease; break; }
            adopt();
            J = Jn;
            if (!(J == J)) { status |= TFMPC_ST_NAN; reason = kReasonFailed; break; }
        }
        if (reason == kReasonPassCap) status |= TFMPC_ST_MAX_ATTEMPTS;
    } else if (status) {
        reason = kReasonFailed;
    }

    if (status & (TFMPC_ST_NOT_PD | TFMPC_ST_NAN)) {
        const S qnan = std::numeric_limits<S>::quiet_NaN();
        for (size_t i = lane; i < nx; i += kWave) xs[i] = qnan;
        for (size_t i = lane; i < nu; i += kWave) us[i] = qnan;
        for (size_t i = lane; i < nc; i += kWave) cs[i] = qnan;
    }
    if (lane == 0) {
        p.iterations[b] = sweeps;
        a.status[b] = status;
        if (p.reason) p.reason[b] = reason;
    }
