// bp_edge_out_status.h -- a syndrome's `iters` and `conv`, and the end of its turn, for every lane = edge min-sum kernel, written once
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT (see bp_edge_check4.h): no include guard, no declarations of its own.  The ten FP64 kernels and
// the two of bp_edge_f32_kernel.h include it as the last thing of their syndrome loop's body.
// It uses the including kernel's b, lane, it (the iterations run), unsat (the syndrome was not reproduced) and LDPC_EDGE_ARG (bp_edge_synd.h).
// The Relay-BP kernels, whose `it` and `unsat` are a leg's, define the two for the row in a block around the #include.
        {
            const auto ip = global_ptr(LDPC_EDGE_ARG(iters));
            const auto cp = global_ptr(LDPC_EDGE_ARG(conv));
            if (lane == 0) {
                if (ip) ip[b] = it;
                if (cp) cp[b] = unsat ? 0 : 1;
            }
        }
        // The wavefront must be whole again before lane 0 pulls the next syndrome: without this (convergent) barrier the
        // compiler threads this `lane == 0` block into the one at the top of the loop and the readfirstlane there runs with
        // lane 0 masked off -- every other lane's `pulled` is 0, i.e. syndrome 0 for ever (seen with R = 1).
        __builtin_amdgcn_wave_barrier();
