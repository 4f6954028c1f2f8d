// bp_edge_bit4_mem.h -- the bit pass of the lane = edge min-sum kernels with columns of weight <= 2 in the MEMORY form, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  bp_edge_mem_kernel and
// bp_edge_relay_kernel include it where the pass stands in their iteration.
// It uses the including kernel's R, KEEP, msg, prv, av, gv, a_t, g_t, paddr, k0, sy, X, lane, bad (a uint64_t it declares as 0 before the
// #include) and namespace edge_detail; no macros.
//
// bp_edge_bit4.h with the prior formed from M = prv[r] and the slot's a and gamma (bp_edge_mem_kernel.h, which also says why that prior is
// never -0.0), and prv[r] <- the column's posterior: the prior from M; the partner's message; log-ratio, decision, new bit_to_check.  Up to
// KEEP rounds a and gamma are registers; above, they are read from the tables beside the partner's message, a group of EDGE_G rounds at a time.
#pragma unroll
            for (int r0 = 0; r0 < R; r0 += EDGE_G) {
                double cpv[EDGE_G], asv[EDGE_G], gsv[EDGE_G];
#pragma unroll
                for (int g = 0; g < EDGE_G; ++g)
                    if (r0 + g < R) {
                        cpv[g] = X[paddr[r0 + g]];
                        asv[g] = KEEP ? av[KEEP ? r0 + g : 0] : a_t[(r0 + g) * 64 + lane];
                        gsv[g] = KEEP ? gv[KEEP ? r0 + g : 0] : g_t[(r0 + g) * 64 + lane];
                    }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < EDGE_G; ++g) {
                    const int r = r0 + g;
                    if (r >= R) break;
                    const double cp = cpv[g];
                    const double c = msg[r];
                    const double pr = gsv[g] == 0.0 ? asv[g] : asv[g] + gsv[g] * prv[r];  // THIS iteration's prior, from M = prv[r]
                    const double b2c = pr + cp;
                    const double l1 = b2c + c;             // second entry of its column: (prior + c0) + c1 with c0 = the partner's
                    const double l0 = (pr + c) + cp;       // first entry: c0 = its own
                    // the column's posterior, the same value in both of its lanes
                    const double l = __hiloint2double(select_by_mask(__double2hiint(l1), __double2hiint(l0), k0[r]),
                                                      select_by_mask(__double2loint(l1), __double2loint(l0), k0[r]));
                    const uint64_t d = __ballot(l <= 0.0);  // (phantom lanes: +inf or NaN, never <= 0)
                    bad |= nibble_parity_low(d) ^ sy[r];  // candidate syndrome vs syndrome (bp.hpp:292-302), bit 0 of every nibble
                    msg[r] = b2c;
                    prv[r] = l;  // M of the next iteration (Relay-BP: and of the next leg); after the last one: the output
                }
            }
