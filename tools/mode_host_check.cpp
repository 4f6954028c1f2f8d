// Stand-alone walk of ldpc_amd/csrc/mode_host.h -- what float32 messages, memory min-sum, Relay-BP and guided decimation refuse, and the setters'
// exclusion messages -- meant to run under the host sanitizers (nothing of it touches a GPU or Python):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//         -I ldpc_amd/csrc tools/mode_host_check.cpp -o mode_host_check
//     ./mode_host_check     (exit status 0, last line "mode_host_check ok"; tests/test_mode_rules.py builds and runs it)
// One line per state, in the order of the loops below: a bare "0" where the decode is accepted, else "<code> <message>".  The test compares the
// lines with tests/golden/mode_rules_c.json, which the hand-written ladders this header replaced answered on the same walk.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mode_host.h"

static void answer(int code, const char *msg) {
    if (code) std::printf("%d %s\n", code, msg);
    else std::printf("0\n");
}

int main() {
    const char *const whats[] = {nullptr, "per-row channel probabilities are", "soft-syndrome decoding is", "decoding over several GPUs (ldpc_hip_bp_multi) is"};
    const struct { bool with_osd; int method, order; } osds[] = {{false, 1, 0}, {true, 1, 0}, {true, 2, 2}, {true, 3, 2}};  // a call without OSD, OSD-0, OSD-E, OSD-CS
    const Variant variants[] = {Variant::Plain, Variant::Memory, Variant::Relay, Variant::Decimation};
    char msg[512];
    for (int method : {LDPC_HIP_PRODUCT_SUM, LDPC_HIP_MINIMUM_SUM})
        for (bool parallel : {true, false})
            for (int dtype : {LDPC_HIP_MSG_F64, LDPC_HIP_MSG_F32})
                for (Variant variant : variants)
                    for (int bad_col : {-1, 3})
                        for (bool route : {true, false})
                            for (const char *what : whats)
                                for (const auto &osd : osds) {
                                    const ModeState s = {method, parallel, dtype, variant, bad_col, route, route ? -1 : 2, osd.method, osd.order};
                                    std::memset(msg, '#', sizeof msg);  // (a refusal writes and ends its own text; an acceptance reads none)
                                    answer(mode_refusal(s, DecodeCall{what, osd.with_osd}, msg, sizeof msg), msg);
                                }
    // the six exclusion pairs of the setters, then what they accept
    for (int wanted = 1; wanted <= 3; ++wanted)
        for (int held = 1; held <= 3; ++held)
            if (held != wanted) answer(mode_exclusion(variants[wanted], variants[held], msg, sizeof msg), msg);
    for (int wanted = 1; wanted <= 3; ++wanted) {
        answer(mode_exclusion(variants[wanted], Variant::Plain, msg, sizeof msg), msg);
        answer(mode_exclusion(variants[wanted], variants[wanted], msg, sizeof msg), msg);
    }
    std::printf("mode_host_check ok\n");
    return 0;
}
