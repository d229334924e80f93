// Overlapping window rows (td_windows.hip): one document per row, a document longer than the row's body room continues in
// further rows of its own, each repeating the last `overlap` ids of the row before.  The contract is in
// include/tokendagger_hip.h (TD_ROWS_WINDOWS).  Kept apart from EncodeArgs / Tables and from RowsArgs: nothing of the encode
// or of the other layouts is touched.  The workgroup size, the tile and the grid cap, and the device helpers shared with the
// other layouts, are in td_rows_common.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_rows_lab.h"

namespace td {

constexpr int WIN_SCAN_HEAD = 4;      // scan words in front of the chunk sums: real slots, split documents, largest w_d, bad offsets

struct WindowArgs {
    const int32_t* ids;       // [n_tokens]
    int64_t n_tokens;         // ids the buffer holds: tok_off[n_docs] above it is an error, no id at or above it is read
    const int64_t* tok_off;   // [n_docs + 1]
    int64_t n_docs;
    int64_t S, C, overlap, step;  // seq_len, body room S - b - e, ids repeated, C - overlap
    unsigned long long s_magic, step_magic;  // floor((2^64 - 1) / S), floor((2^64 - 1) / step): x / S and x / step without a 64-bit division
    int32_t bos, eos, pad;
    int b, e;                 // bos / eos present
    int32_t* out;             // [rows_cap * S]
    int64_t rows_cap;
    int32_t* pos;             // [rows_cap * S] or null
    int32_t* row_len;         // [rows_cap] or null
    int64_t* row_doc;         // [rows_cap] or null
    int64_t* row_start;       // [rows_cap] or null
    long long* counts;        // [4] rows, real slots, documents with more than one window, the largest w_d
    unsigned long long* scan; // [WIN_SCAN_HEAD + chunks]: the head (zeroed before the launch), then every chunk's rows / exclusive prefix
    int64_t* first_row;       // [n_docs + 1] exclusive prefix sum of w_d; [n_docs] = rows, or -1 when the offsets are invalid
    int* err;
    long long* err_pos;
};

// What the host fills and the launchers take: WindowArgs, and behind it the label stream of the pair form (lab.src null: one stream).
// The one-stream kernels get the WindowArgs slice alone, so that their arguments are what they were without the pair form.
struct WindowLabArgs : WindowArgs {
    LabArgs lab;
};

// td_win_count, td_win_chunks, td_win_first (the window counts and their scan), then td_win_slots.  The caller zeroes
// scan[0, WIN_SCAN_HEAD) on the same stream first.
hipError_t launch_windows(const WindowLabArgs& a, hipStream_t stream);
int64_t windows_scan_words(int64_t n_docs);

}  // namespace td
