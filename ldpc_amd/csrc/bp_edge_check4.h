// bp_edge_check4.h -- the check pass of the lane = edge min-sum kernels whose rows sit in FOUR neighbouring lanes, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT, not a header: no include guard, no declarations of its own.  bp_edge_kernel,
// bp_edge_rp_kernel, bp_edge_mem_kernel, bp_edge_relay_kernel and bp_edge_gd_kernel include it where the pass stands in their iteration, so
// each compiles the token stream it had when the pass was written out in it, and so the same code (profiles/edge_fragments_isa.txt; as
// __forceinline__ function templates the passes compiled to other code: profiles/edge_passes_isa.txt).
// It uses the including kernel's R, NOCLAMP (a constexpr bool: bp_edge_kernel's template parameter, `false` in the variants), msg, sy, al,
// dbl_max, X, lane and namespace edge_detail (bp_edge_kernel.h); no macros.
//
// msg[r] (bit_to_check) -> msg[r] (check_to_bit), stored at the slot (bp.hpp:220-273).  A row's (up to) four entries sit in four
// neighbouring lanes: two DPP quad permutations bring the minimum over the three OTHER entries, one ballot and scalar bit tricks on the
// 64-bit lane mask the row's sign parity.
// The reference's minimum starts from DBL_MAX and replaces it only by something SMALLER (bp.hpp:240-247): an infinite |bit_to_check| never
// enters it.  Hence the clamp min(., DBL_MAX) after the butterfly -- and hence phantom lanes (a row lighter than four, the padding behind the
// last row) may hold +inf for good (prior +inf, partner = a slot that holds +inf): clamped to DBL_MAX in the minimum, positive in the sign
// ballot, and their "log-ratio" is +inf or, at worst, inf - inf = NaN: never <= 0, so they drop out of the decision ballots by themselves.
// NOCLAMP: the clamp cannot bite and is left out; when that is so is argued at bp_edge_kernel, the one kernel that has the parameter.
// The first EDGE_V1 (NOCLAMP: EDGE_V1N) rounds spread the row's parity on the vector unit, the others on the scalar unit: the balance is
// measured (bp_edge_kernel.h, where the constants are).
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double cur = msg[r];
                const uint64_t neg = __ballot(cur <= 0.0);
                const double x1 = quad_perm<0xB1>(cur);               // lane ^ 1
                const double pairmin = min_abs(cur, x1);
                const double other = quad_perm<0x4E>(pairmin);        // the other pair's minimum (lane ^ 2)
                const double mag = NOCLAMP ? min_abs(x1, other) : fmin_pos(min_abs(x1, other), dbl_max);  // over the three other entries, from DBL_MAX down
                int shi;  // high word of +-alpha: sign = row parity (syndrome included) + own
                if (r < (NOCLAMP ? EDGE_V1N : EDGE_V1)) {
                    // the vector unit spreads the row's parity: lane 0 of the quad picks it up from the (unspread) scalar mask, a DPP
                    // broadcast inside the quad XORs it onto everyone's own sign -- 2 vector instructions more, 5 scalar ones fewer
                    const uint64_t par = nibble_parity_low(neg ^ sy[r]);
                    const int own = select_by_mask(al.hi, al.nhi, neg);
                    const int rowbit = select_by_mask(0, (int)0x80000000, par);
                    shi = own ^ __builtin_amdgcn_mov_dpp(rowbit, 0x00, 0xf, 0xf, true);  // quad_perm [0, 0, 0, 0]
                } else {
                    const uint64_t flip = spread_nibble(nibble_parity_low(neg ^ sy[r])) ^ neg;  // row parity incl. the syndrome, own sign out
                    shi = select_by_mask(al.hi, al.nhi, flip);
                }
                const double c = mag * __hiloint2double(shi, al.lo);
                msg[r] = c;
                X[r * 64 + lane] = c;
            }
