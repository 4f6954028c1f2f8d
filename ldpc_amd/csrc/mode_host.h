// mode_host.h -- what each decode mode refuses, stated once: float32 messages, memory min-sum, Relay-BP, guided decimation
// Plain C++ with no HIP in it, so that a stand-alone program can include it and run under a host sanitizer (tools/mode_host_check.cpp);
// host_handle.h (decode_gate) and host_setup.h (the three setters) are the only other users.  A new mode is a row of k_mode_rules, a value of
// Variant if the handle holds it instead of the other three, and -- only if it brings a rule no row has yet -- a column and its line in mode_refusal.
#pragma once

#include <cstddef>
#include <cstdio>

#include "../../include/ldpc_hip.h"

// What the handle decodes with besides plain BP: at most one of the three (the setters refuse a second: mode_exclusion).
enum class Variant { Plain, Memory, Relay, Decimation };

struct ModeRules {
    const char *label;       // opens every message of the mode
    const char *noun;        // "switch <noun> off" (nullptr: float32, whose remedy is `off` alone)
    const char *off;         // the call that switches it off
    // why a decode is refused, in the order they are asked; nullptr: the rule does not apply to the mode
    const char *product_sum, *serial, *float32;
    const char *bad_column;  // %d: the column -- a nonzero memory strength on a channel probability of 0 or 1
    const char *no_route;    // %d: the small-code kernel mode -- no lane = edge family takes the code
    bool osd0_only;          // OSD-E and OSD-CS after it are refused
    const char *no_route_node = nullptr;  // %d: the mode -- no_route's text where the lane = node route was asked for too (ModeState::lane_node)
};

#define LDPC_MODE_SERIAL "the serial schedules are not available (parallel schedule required)"
#define LDPC_MODE_FLOAT32 "float32 messages are not available (set the message dtype to float64)"
#define LDPC_MODE_PS_MEMORY "product-sum is not available (the memory strengths are defined for minimum-sum only)"
#define LDPC_MODE_BAD_COLUMN "column %d has a nonzero memory strength and a channel probability of 0 or 1 -- it needs probabilities strictly between 0 and 1 "
// row 0: float32 messages; rows 1 .. 3: by Variant
static const ModeRules k_mode_rules[4] = {
    {"float32 messages", nullptr, "set the message dtype to float64",
     "product-sum is not available (its tanh / log have no bit-exact FP32 form here); use minimum-sum or float64", LDPC_MODE_SERIAL, nullptr, nullptr, nullptr, false},
    {"memory min-sum", "the memory", "ldpc_hip_bp_set_memory(h, NULL)",
     LDPC_MODE_PS_MEMORY, LDPC_MODE_SERIAL, LDPC_MODE_FLOAT32, LDPC_MODE_BAD_COLUMN "(or strength 0 on that column)", nullptr, false},
    {"Relay-BP", "the relay", "ldpc_hip_bp_set_relay(h, 0, NULL, NULL, 0)",
     LDPC_MODE_PS_MEMORY, LDPC_MODE_SERIAL, LDPC_MODE_FLOAT32, LDPC_MODE_BAD_COLUMN "(or strength 0 on that column in every leg)", nullptr, true},
    {"guided decimation", "the decimation", "ldpc_hip_bp_set_decimation(h, 0, 0, 0)",
     "product-sum is not available (it is built on the minimum-sum lane = edge kernels only)", LDPC_MODE_SERIAL, LDPC_MODE_FLOAT32, nullptr,
     "neither lane = edge kernel family takes this code under small-code kernel mode %d "
     "(ldpc_hip_bp_decimation_route answers 0: it needs rows of at most 8 and columns of at most 4 entries within the kernels' ladders, and mode -1, 1 or 6); "
     "the lane = node route for larger codes and a per-pass route are not built yet", true,
     "neither lane = edge kernel family nor the lane = node kernel takes this code under small-code kernel mode %d "
     "(ldpc_hip_bp_decimation_route answers 0: the lane = node kernel needs rows of at most 16 and columns of at most 8 entries, a syndrome's state "
     "within LDS, and mode -1, 1, 3, 4 or 5); a per-pass route is not built"},
};

// What a handle is set up for, as far as the rules look at it.
struct ModeState {
    int bp_method;      // LDPC_HIP_PRODUCT_SUM | LDPC_HIP_MINIMUM_SUM
    bool parallel;      // the parallel schedule, and not random-serial
    int msg_dtype;      // LDPC_HIP_MSG_F64 | LDPC_HIP_MSG_F32
    Variant variant;
    int bad_col;        // the variant's first column with a nonzero strength on a probability of 0 or 1 (-1: none)
    bool route;         // an on-chip kernel takes the code (asked of guided decimation only)
    int small_mode, osd_method, osd_order;  // the small-code kernel mode (no_route's message); the handle's OSD
    bool lane_node = false;  // guided decimation: the lane = node route is switched on (ldpc_hip_bp_set_decimation_lane_node) -- which sentence a missing route gets
};

// What a decode entry point adds: `what` -- "per-row channel probabilities are", "soft-syndrome decoding is", ... -- is something no mode does
// (nullptr: a plain call); with_osd: the call runs the handle's osd_method / osd_order.
struct DecodeCall { const char *what; bool with_osd; };

// 0, or LDPC_HIP_ERR_UNSUPPORTED with the reason in msg: float32 messages speak first, then the variant -- each its `what` sentence or the first
// of its rules the state breaks -- then OSD of a higher order than OSD-0 (osd_order 0 takes the OSD-0 branch whatever the method).
inline int mode_refusal(const ModeState &s, const DecodeCall &call, char *msg, size_t cap) {
    const bool f32 = s.msg_dtype == LDPC_HIP_MSG_F32;
    const ModeRules *const on[2] = {f32 ? &k_mode_rules[0] : nullptr, s.variant != Variant::Plain ? &k_mode_rules[(int)s.variant] : nullptr};
    for (const ModeRules *r : on) {
        if (!r) continue;
        const size_t head = (size_t)snprintf(msg, cap, "%s: ", r->label), room = cap - head;  // (a label is a few words: head < cap)
        char *const at = msg + head;
        if (call.what && r->noun) snprintf(at, room, "%s not available (switch %s off: %s)", call.what, r->noun, r->off);
        else if (call.what) snprintf(at, room, "%s not available (%s)", call.what, r->off);
        else if (r->product_sum && s.bp_method != LDPC_HIP_MINIMUM_SUM) snprintf(at, room, "%s", r->product_sum);
        else if (r->serial && !s.parallel) snprintf(at, room, "%s", r->serial);
        else if (r->float32 && f32) snprintf(at, room, "%s", r->float32);
        else if (r->bad_column && s.bad_col >= 0) snprintf(at, room, r->bad_column, s.bad_col);
        else if (r->no_route && !s.route) snprintf(at, room, s.lane_node && r->no_route_node ? r->no_route_node : r->no_route, s.small_mode);
        else continue;
        return LDPC_HIP_ERR_UNSUPPORTED;
    }
    if (on[1] && on[1]->osd0_only && call.with_osd && s.osd_method >= 2 && s.osd_order > 0) {
        snprintf(msg, cap, "%s: OSD-E and OSD-CS are not available (OSD-0 only: ldpc_hip_bp_set_osd(h, 1, 0), or switch %s off)", on[1]->label, on[1]->noun);
        return LDPC_HIP_ERR_UNSUPPORTED;
    }
    return LDPC_HIP_OK;
}

// A setter switching `wanted` on while the handle holds `held`: 0 (nothing held, or the same variant set anew), or LDPC_HIP_ERR_UNSUPPORTED.
inline int mode_exclusion(Variant wanted, Variant held, char *msg, size_t cap) {
    if (held == Variant::Plain || held == wanted) return LDPC_HIP_OK;
    const ModeRules &w = k_mode_rules[(int)wanted], &o = k_mode_rules[(int)held];
    snprintf(msg, cap, "%s and %s exclude each other: switch %s off first (%s)", w.label, o.label, o.noun, o.off);
    return LDPC_HIP_ERR_UNSUPPORTED;
}
