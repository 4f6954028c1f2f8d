// bp_edge_relay_take.h -- what the lane = edge Relay-BP kernels do with a leg's parked posteriors, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  bp_edge_relay_kernel and
// bp_edge8_relay_kernel include it at a leg's end -- a solution, or the last leg of a row without one -- after they have parked prv[] at
// X[column], each in its own way.
// It uses the including kernel's X, b, n, lane, unsat, the row's running best and nsol, ARGS_T (for llr0) and LDPC_EDGE_ARG (bp_edge_synd.h).
// A solution's weight is formed from the parked posteriors (relay_weight: lanes stride the columns, a butterfly over the wavefront); if it is
// strictly smaller than the best so far, the row's decoding and llr go to global memory, over an earlier solution's.  A row without any
// solution writes the last leg's last bit pass.
                bool take = unsat;
                if (!unsat) {
                    const double w = relay_weight((const double *)LDPC_KERNARG(ARGS_T, llr0), n, lane, [&](int j) { return X[j] <= 0.0; });
                    ++nsol;
                    if (__ballot(w < best) != 0) { best = w; take = true; }  // (every lane holds the same w: the ballot keeps the branch scalar)
                }
                if (take) {
#include "bp_edge_out_rows.h"
                }
