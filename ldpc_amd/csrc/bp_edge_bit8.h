// bp_edge_bit8.h -- the bit pass of the lane = edge min-sum kernels with columns of weight <= DC, in the plain and in the memory form, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  bp_edge8_kernel,
// bp_edge8_rp_kernel and bp_edge8_gd_kernel include it where the pass stands in their iteration in the plain form, bp_edge8_mem_kernel and
// bp_edge8_relay_kernel in the memory form.
// It uses the including kernel's R, DC, msg, caddr, kmask, sy, X, bad (a uint64_t it declares as 0 before the #include) and namespace
// edge_detail; in the memory form also prv, KEEP, av, gv, a_t, g_t and lane.  One macro decides the form:
//   LDPC_EDGE_PRIOR(r)   defined: the plain form -- it is the prior of the lane's column in round r, and the pass leaves it alone;
//                        not defined: the memory form -- the prior is formed from M = prv[r] and the slot's a and gamma
//                        (bp_edge_mem_kernel.h), and prv[r] <- the column's posterior
//
// The column's entries in order; log-ratio, decision, the lane's own bit_to_check (bp.hpp:276-318).  A lane reads ALL entries of its column
// from the wave-private LDS array in column order (its own included; lighter columns: the +0.0 slot behind their entries) and forms the
// reference's sums with them:
//     log-ratio            (((prior + c0) + c1) + c2) + c3                                   (bp.hpp:278-281), the same in every lane of a column,
//     bit_to_check of k    ((prior + c0) + ... + c_{k-1})  +  (((0 + c_{DC-1}) + ...) + c_{k+1})  (bp.hpp:279, 311-318)
// (0.0 + x and x + 0.0 are dropped where x + a prior follows or the sum contains the prior: they can only turn -0.0 into +0.0, which a sum
// with a prior that is never -0.0 does not see); the lane's own k picks its bit_to_check by two or three v_cndmask pairs reading per-round
// lane masks from SGPRs.
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double c[DC];
#pragma unroll
                for (int j = 0; j < DC; ++j) c[j] = X[caddr[r][j]];
#ifndef LDPC_EDGE_PRIOR
                const double as = KEEP ? av[KEEP ? r : 0] : a_t[r * 64 + lane], gs = KEEP ? gv[KEEP ? r : 0] : g_t[r * 64 + lane];
                if (!KEEP && (r & 1)) __builtin_amdgcn_sched_barrier(0);  // (two rounds' table reads in flight, not all R: they would cost 4 R registers)
                const double pr = gs == 0.0 ? as : as + gs * prv[r];  // THIS iteration's prior, from M = prv[r]
#else
                const double pr = LDPC_EDGE_PRIOR(r);
#endif
                double pre[DC];  // pre[k] = prior + c0 + ... + c_{k-1}
                double t = pr;
#pragma unroll
                for (int j = 0; j < DC; ++j) { pre[j] = t; t += c[j]; }
                const uint64_t d = __ballot(t <= 0.0);  // (phantom lanes: +inf or NaN, never <= 0)
                bad |= byte_parity_low(d) ^ sy[r];
                // the lane's own bit_to_check: cand[k] = pre[k] + (((0 + c_{DC-1}) + ...) + c_{k+1}), accumulated downwards as the reference
                // does (bp.hpp:311-318); the k-th entry of its column takes cand[k]
                double cand[DC];
                double sfx = c[DC - 1];
                cand[DC - 1] = pre[DC - 1];
                cand[DC - 2] = pre[DC - 2] + sfx;
#pragma unroll
                for (int k = DC - 3; k >= 0; --k) { sfx += c[k + 1]; cand[k] = pre[k] + sfx; }
                double b2c = cand[0];
#pragma unroll
                for (int k = 1; k < DC; ++k) b2c = select_f64(b2c, cand[k], kmask[r][k - 1]);
                msg[r] = b2c;
#ifndef LDPC_EDGE_PRIOR
                prv[r] = t;  // M: the forward sum's end value, the same in every lane of the column
#endif
            }
