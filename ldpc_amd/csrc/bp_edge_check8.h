// bp_edge_check8.h -- the check pass of the lane = edge min-sum kernels whose rows sit in EIGHT neighbouring lanes, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  bp_edge8_kernel,
// bp_edge8_rp_kernel, bp_edge8_mem_kernel, bp_edge8_relay_kernel and bp_edge8_gd_kernel include it where the pass stands in their iteration.
// It uses the including kernel's R, msg, sy, al, dbl_max, X, lane and namespace edge_detail (bp_edge_kernel.h); no macros.
//
// msg[r] (bit_to_check) -> msg[r] (check_to_bit), stored at the slot (bp.hpp:220-273): the minimum over the SEVEN other lanes of the group,
// the sign by the group's parity.  Against bp_edge_check4.h the butterfly has a third step across the two quads of the 8-lane group
// (xor4: row_shl:4 / row_shr:4 DPP moves, each writing the banks it is meant for), and the sign parity is a BYTE parity of the lane mask.
// The clamp to DBL_MAX and the phantom lanes: as argued in bp_edge_check4.h.
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double cur = msg[r];
                const uint64_t neg = __ballot(cur <= 0.0);
                const double x1 = quad_perm<0xB1>(cur);                // lane ^ 1
                const double pairmin = min_abs(cur, x1);
                const double otherpair = quad_perm<0x4E>(pairmin);     // lane ^ 2: the other pair of the quad
                const double inquad = min_abs(x1, otherpair);          // the three others of the quad
                const double quadmin = min_abs(pairmin, otherpair);    // ... and the whole quad, for the other quad (values >= 0: |.| is idle)
                const double otherquad = xor4(quadmin);
                const double mag = fmin_pos(min_abs(inquad, otherquad), dbl_max);  // the seven other entries, from DBL_MAX down
                const uint64_t flip = spread_byte(byte_parity_low(neg ^ sy[r])) ^ neg;
                const double c = mag * __hiloint2double(select_by_mask(al.hi, al.nhi, flip), al.lo);
                msg[r] = c;
                X[r * 64 + lane] = c;
            }
