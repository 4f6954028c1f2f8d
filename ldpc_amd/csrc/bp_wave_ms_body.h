// bp_wave_ms_body.h -- the body of one min-sum iteration on the lane = node layout, written once for bp_wave_relay_kernel and bp_wave_gd_kernel
// Part of libldpc_hip.so.  A TEXTUAL FRAGMENT, not a header: no include guard, no declarations of its own.  bp_wave_relay_kernel.h and
// bp_wave_gd_kernel.h include it as the body of their `do { ... } while (unsat_any && it < ...)`, so each kernel compiles the token stream it
// had when the passes were written out in it, and so the same code (profiles/wave_body_isa.txt: a function template did not keep it).
// The iteration: ++it, alpha, the min-sum check pass, the bit pass, the syndrome test and TEAM's two flags of bp_wave_kernel
// (bp_wave_kernel.h), operation by operation.  It uses the including kernel's DR, DC, TEAM, U, UC, a, it, unsat_any, lane, tid, wt, W, mp, np,
// M, L, hardw, sy, rdeg, col, apos, DUMMY, ZERO, team_unsat, team_sync, and two macros the kernel defines before the #include (undefined here):
//   WAVE_MS_SET_PRIOR(pr, j, word)  a statement that sets pr, the prior of column j in the bit pass; word = j / 64, the same for the wavefront
//   WAVE_MS_ITERATIONS              the iterations of the syndrome so far, this one included: what TEAM's flags go by
                ++it;
                const double alpha = (a.ms_scaling_factor == 0.0) ? 1.0 - ldexp(1.0, -it) : a.ms_scaling_factor;
                // ---- check pass (bp.hpp:201-273), in place, UC rows per lane in flight: loads, arithmetic, stores ----
                for (int i0 = wt * 64 * UC; i0 < mp; i0 += 64 * UC * W) {
                    uint8_t sb[UC];
                    int d[UC];
                    double cur[UC][DR], out[UC][DR];
#pragma unroll
                    for (int u = 0; u < UC; ++u)
                        if (i0 + u * 64 < mp) {  // wave-uniform
                            const int i = i0 + u * 64 + lane;
                            sb[u] = sy[i];
                            d[u] = rdeg[i];
#pragma unroll
                            for (int k = 0; k < DR; ++k) cur[u][k] = M[k * mp + i];
                        }
#pragma unroll
                    for (int u = 0; u < UC; ++u)
                        if (i0 + u * 64 < mp) {
                            int parity = sb[u] & 1;  // total_sgn = syndrome[i] + #{b2c <= 0}, parity only (bp.hpp:236-262)
                            double temp = DBL_MAX;
#pragma unroll
                            for (int k = 0; k < DR; ++k) {
                                if (cur[u][k] <= 0) parity ^= 1;
                                out[u][k] = temp;
                                const double ab = fabs(cur[u][k]);
                                if (ab < temp) temp = ab;
                            }
                            temp = DBL_MAX;
#pragma unroll
                            for (int k = DR - 1; k >= 0; --k) {
                                const int sgn = parity ^ (cur[u][k] <= 0 ? 1 : 0);
                                double mag = out[u][k];
                                if (temp < mag) mag = temp;
                                out[u][k] = mag * (sgn ? -alpha : alpha);
                                const double ab = fabs(cur[u][k]);
                                if (ab < temp) temp = ab;
                            }
                        }
#pragma unroll
                    for (int u = 0; u < UC; ++u)
                        if (i0 + u * 64 < mp) {
                            const int i = i0 + u * 64 + lane;
#pragma unroll
                            for (int k = 0; k < DR; ++k) M[k < d[u] ? k * mp + i : DUMMY] = out[u][k];  // phantom entries keep their neutral value
                        }
                }
                team_sync();
                // ---- bit pass (bp.hpp:276-298, 311-318), in place through the position table, U bits per lane in flight; the prior is the kernel's ----
                for (int j0 = wt * 64 * U; j0 < np; j0 += 64 * U * W) {
                    int pos[U][DC];
                    double c[U][DC], pre[U][DC], pr[U];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j0 + u * 64 < np) {
                            const int j = j0 + u * 64 + lane;
                            WAVE_MS_SET_PRIOR(pr[u], j, (j0 >> 6) + u)
#pragma unroll
                            for (int k = 0; k < DC; ++k) { pos[u][k] = apos[k * np + j]; c[u][k] = M[pos[u][k]]; }  // phantom: the +0.0 slot
                        }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j0 + u * 64 < np) {
                            double temp = pr[u];
#pragma unroll
                            for (int k = 0; k < DC; ++k) { pre[u][k] = temp; temp += c[u][k]; }
                            L[j0 + u * 64 + lane] = temp;  // the posteriors: the relay's memory, what a decimation looks at, the outputs
                            const uint64_t word = __ballot(temp <= 0);  // padding bits: prior 1.0, no entries -> 0
                            if (lane == 0) hardw[(j0 >> 6) + u] = word;
                            double sfx = 0.0;
#pragma unroll
                            for (int k = DC - 1; k >= 0; --k) {
                                pre[u][k] = pre[u][k] + sfx;
                                sfx += c[u][k];
                            }
                        }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j0 + u * 64 < np) {
#pragma unroll
                            for (int k = 0; k < DC; ++k) M[pos[u][k] == ZERO ? DUMMY : pos[u][k]] = pre[u][k];
                        }
                }
                team_sync();
                // ---- syndrome test (bp.hpp:292-294, 300-302): candidate parity of every check vs its syndrome BYTE ----
                bool unsat = false;
                for (int i0 = wt * 64; i0 < mp; i0 += 64 * W) {
                    const int i = i0 + lane;
                    unsigned par = 0;
#pragma unroll
                    for (int k = 0; k < DR; ++k) {
                        const int cj = col[k * mp + i];  // phantom: bit np, always zero
                        par ^= (unsigned)(hardw[cj >> 6] >> (cj & 63)) & 1u;
                    }
                    unsat |= par != (unsigned)sy[i];
                }
                unsat_any = __ballot(unsat) != 0;
                if (TEAM) {  // two flags, by the syndrome's iterations so far: iteration g + 1 raises the one nobody has read since iteration g - 1
                    const int g = WAVE_MS_ITERATIONS;
                    if (unsat_any && lane == 0) team_unsat[g & 1] = 1;
                    if (tid == 0) team_unsat[(g + 1) & 1] = 0;
                    __syncthreads();
                    unsat_any = team_unsat[g & 1] != 0;
                }
#undef WAVE_MS_SET_PRIOR
#undef WAVE_MS_ITERATIONS
