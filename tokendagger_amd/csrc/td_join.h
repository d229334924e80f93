// Field joins (td_join.hip): ids + per-document token offsets, K documents an example -> one output document an example, literal
// ids between the fields, per-field and per-example truncation, and a label and a type stream written in the same pass.  The
// contract is in include/tokendagger_hip.h (td_join_spec); the truncation rule, shared with td_join_plan, in td_join_args.h.
// The workgroup size, the tile and the grid cap, and the device helpers shared with the row layouts, are in td_rows_common.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_join_args.h"

namespace td {

// scan words in front of the chunk sums (two a chunk: kept examples, kept slots)
enum { JOIN_N_DROPPED = 0, JOIN_N_TRUNC = 1, JOIN_BAD = 2, JOIN_LEAVE = 3, JOIN_E = 4, JOIN_T = 5, JOIN_SCAN_HEAD = 8 };

struct JoinArgs {
    const int32_t* ids;       // [n_tokens]
    int64_t n_tokens;         // ids the buffer holds: no id at or above it is read
    const int64_t* tok_off;   // [n_ex * K + 1]
    int64_t n_ex;
    JoinRule rule;
    int32_t lit[JOIN_MAX_FIELDS + 1][JOIN_MAX_LITERAL];  // before_f at f, the tail at K
    int32_t type_of[JOIN_MAX_FIELDS + 1];                // type_value of field f, tail_type at K
    uint32_t train;           // bit p: part p (before_f = 2f, body_f = 2f + 1, tail = 2K) is trained
    int32_t ignore_index;
    int32_t* out;             // [ids_cap]
    int32_t* out_labels;      // [ids_cap] or null
    int32_t* out_types;       // [ids_cap] or null
    int64_t ids_cap;
    int64_t* out_off;         // [n_ex + 1], E + 1 written
    int64_t* out_examples;    // [n_ex] or null, E written
    int32_t* out_field_len;   // [n_ex * K] or null, E * K written
    long long* counts;        // [4] E, T, examples dropped, examples truncated
    unsigned long long* scan; // [JOIN_SCAN_HEAD + 2 * chunks]: the head (zeroed before the launch), then every chunk's sums / exclusive prefixes
    int64_t* plan;            // [n_ex * join_plan_words(K)] a record a kept example: the starts of its 2K + 1 parts inside it, then the
                              // source index of each body's first kept id
    int* err;
    long long* err_pos;
};

// td_join_count, td_join_chunks, td_join_first (what is kept, its lengths and its scan), then td_join_slots.  The caller zeroes
// scan[0, JOIN_SCAN_HEAD) on the same stream first.
hipError_t launch_join(const JoinArgs& a, hipStream_t stream);
int64_t join_scan_words(int64_t n_ex);
constexpr int64_t join_plan_words(int K) { return 3 * (int64_t)K + 1; }

}  // namespace td
