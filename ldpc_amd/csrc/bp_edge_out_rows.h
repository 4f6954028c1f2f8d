// bp_edge_out_rows.h -- a syndrome's decoding and log-ratios leave the chip, for the FP64 lane = edge min-sum kernels, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  Every FP64 kernel
// includes it after it has parked the log-ratio of column j at X[j] (n <= R * 64: every column has an entry, and the next syndrome's first
// check pass rewrites every slot) -- the two Relay-BP kernels through bp_edge_relay_take.h, when a leg's result is taken.
// It uses the including kernel's X, b, n, lane and LDPC_EDGE_ARG (bp_edge_synd.h).
// Outputs (bp.hpp:62,65,69,71) in whole 512- / 64-byte rows.
        {
            const auto dp = global_ptr(LDPC_EDGE_ARG(decoding)) + (int64_t)b * n;
            auto lp = global_ptr(LDPC_EDGE_ARG(llr));
            if (lp) lp += (int64_t)b * n;
            for (int j = lane; j < n; j += 64) {
                const double t = X[j];
                dp[j] = t <= 0.0 ? 1 : 0;
                if (lp) lp[j] = t;
            }
        }
