// Document selection (td_select.hip): ids + per-document token offsets + a list of document indices -> the listed documents'
// ids, concatenated in the list's order, with their own offsets; entries whose document is shorter than min_len or longer
// than max_len are dropped.  The contract is in include/tokendagger_hip.h (td_select_spec).  Kept apart from the row layouts'
// arguments: the output is again ids + tok_offsets, what every one of them takes.  The workgroup size, the tile and the grid
// cap, and the device helpers shared with the row layouts, are in td_rows_common.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_rows_lab.h"

namespace td {

// scan words in front of the chunk sums (two a chunk: kept entries, kept ids)
enum { SEL_SHORT = 0, SEL_LONG = 1, SEL_BAD = 2, SEL_LEAVE = 3, SEL_K = 4, SEL_T = 5, SEL_SCAN_HEAD = 8 };

struct SelectArgs {
    const int32_t* ids;       // [n_tokens]
    int64_t n_tokens;         // ids the buffer holds: no id at or above it is read
    const int64_t* tok_off;   // [n_docs + 1]
    int64_t n_docs;
    const int64_t* sel;       // [n_sel] document indices; null: 0 .. n_sel - 1
    int64_t n_sel;
    int64_t min_len, max_len; // max_len < 0: no limit
    int32_t* out;             // [ids_cap]
    int64_t ids_cap;
    int64_t* out_off;         // [n_sel + 1], K + 1 written
    int64_t* out_docs;        // [n_sel] or null, K written
    long long* counts;        // [4] K, T, entries below min_len, entries above max_len
    unsigned long long* scan; // [SEL_SCAN_HEAD + 2 * chunks]: the head (zeroed before the launch), then every chunk's sums / exclusive prefixes
    int64_t* src_base;        // [n_sel] tok_off[out_docs[k]]
    int* err;
    long long* err_pos;
};

// What the host fills and the launcher takes: SelectArgs, and behind it the label stream (lab.src null: one stream; of LabArgs
// only src and dst are used).  The one-stream kernel gets the SelectArgs slice alone.
struct SelectLabArgs : SelectArgs {
    LabArgs lab;
};

// td_sel_count, td_sel_chunks, td_sel_first (what is kept and its scan), then td_sel_slots.  The caller zeroes
// scan[0, SEL_SCAN_HEAD) on the same stream first.
hipError_t launch_select(const SelectLabArgs& a, hipStream_t stream);
int64_t select_scan_words(int64_t n_sel);

}  // namespace td
