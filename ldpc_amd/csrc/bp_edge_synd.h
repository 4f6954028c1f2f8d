// bp_edge_synd.h -- a syndrome's bytes as lane masks, for every lane = edge min-sum kernel, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  The ten FP64 kernels and
// the two of bp_edge_f32_kernel.h include it at the head of their syndrome loop.  It DECLARES sy[R] and never for the rest of the loop body.
// It uses the including kernel's R, LG (a constexpr int: a row sits in 1 << LG neighbouring lanes -- 2 or 3), LOW (bit 0 of every such
// group), b, m, lane, and one macro the kernel's header defines first:
//   LDPC_EDGE_ARG(field)   a cold field of the EdgeArgs / Edge8Args block in the kernel's arguments (bp_edge_kernel.h)
//
// Bit (q << LG) of sy[r] = (byte & 1) of the row that lanes (q << LG) .. ((q + 1) << LG) - 1 serve in round r (kept in bit 0 of every
// group only: one set of masks for both passes); a byte above 1 can never be matched (bp.hpp:300): never.
        uint64_t sy[R];
        bool never = false;
        const auto sb = global_ptr(LDPC_EDGE_ARG(synd)) + (int64_t)b * m;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r * (64 >> LG) + (lane >> LG);
            const int byte = row < m ? (int)sb[row] : 0;
            sy[r] = __ballot((byte & 1) != 0) & LOW;
            never = never || __ballot(byte > 1) != 0;
        }
