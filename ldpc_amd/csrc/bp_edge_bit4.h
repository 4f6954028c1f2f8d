// bp_edge_bit4.h -- the bit pass of the lane = edge min-sum kernels with columns of weight <= 2 and a prior that an iteration leaves alone, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  bp_edge_kernel,
// bp_edge_rp_kernel and bp_edge_gd_kernel include it where the pass stands in their iteration (the memory form: bp_edge_bit4_mem.h).
// It uses the including kernel's R, msg, paddr, k0, sy, X, bad (a uint64_t it declares as 0 before the #include) and namespace edge_detail,
// and one macro the kernel defines first:
//   LDPC_EDGE_PRIOR(r)   the prior of the lane's column in round r (bp_edge_kernel: the scalar or prv[r] by UNIFORM; the variants: prv[r])
//
// The partner's message; log-ratio, decision, new bit_to_check (bp.hpp:276-318).  Column entries c0 (lower row), c1:
//   log-ratio = (prior + c0) + c1 (bp.hpp:278-281);  bit_to_check_0 = prior + (0.0 + c1), bit_to_check_1 = (prior + c0) + 0.0 (bp.hpp:279, :313-316).
// Both equal prior + (the other entry) EXACTLY: x + 0.0 differs from x only for x = -0.0, and neither 0.0 + c1 feeding a sum with the prior
// nor prior + c0 can be a -0.0 that matters -- the prior is log((1 - p) / p), never -0.0, and a sum is -0.0 only if both terms are.  A column
// of weight one reads a slot that holds +0.0 for good: prior + 0.0.  (A variant whose prior is something else says why it is never -0.0.)
// Groups of EDGE_G rounds: their LDS reads are issued together, then consumed -- one round trip per group, not per round.
#pragma unroll
            for (int r0 = 0; r0 < R; r0 += EDGE_G) {
                double cpv[EDGE_G];
#pragma unroll
                for (int g = 0; g < EDGE_G; ++g)
                    if (r0 + g < R) cpv[g] = X[paddr[r0 + g]];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < EDGE_G; ++g) {
                    const int r = r0 + g;
                    if (r >= R) break;
                    const double cp = cpv[g];
                    const double c = msg[r];
                    const double b2c = LDPC_EDGE_PRIOR(r) + cp;
                    const double l1 = b2c + c;                       // second entry of its column: (prior + c0) + c1 with c0 = the partner's
                    const double l0 = (LDPC_EDGE_PRIOR(r) + c) + cp; // first entry: c0 = its own
                    uint64_t d;
                    if (r < EDGE_V2) {  // the vector unit picks the lane's own log-ratio: 1 vector instruction more, 3 scalar ones fewer
                        const double l = __hiloint2double(select_by_mask(__double2hiint(l1), __double2hiint(l0), k0[r]),
                                                          select_by_mask(__double2loint(l1), __double2loint(l0), k0[r]));
                        d = __ballot(l <= 0.0);
                    } else {
                        const uint64_t d1 = __ballot(l1 <= 0.0);
                        d = d1 ^ ((__ballot(l0 <= 0.0) ^ d1) & k0[r]);  // (phantom lanes: neither)
                    }
                    bad |= nibble_parity_low(d) ^ sy[r];  // candidate syndrome vs syndrome (bp.hpp:292-302), bit 0 of every nibble
                    msg[r] = b2c;
                }
            }
