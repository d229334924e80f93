// Training rows from encoded documents (td_rows.hip): ids + per-document token offsets -> fixed-length rows of S slots, with
// BOS / EOS framing and padding, position ids and cu_seqlens (CONCAT) or lengths (PAD).  The contract is in
// include/tokendagger_hip.h (td_make_rows).  Kept apart from EncodeArgs / Tables: nothing of the encode is touched.  The workgroup
// size, the tile and the grid cap, and the device helpers shared with the other layouts, are in td_rows_common.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_rows_lab.h"

namespace td {

struct RowsArgs {
    const int32_t* ids;       // [n_tokens]
    int64_t n_tokens;         // ids the buffer holds: tok_off[n_docs] above it is an error, no id at or above it is read
    const int64_t* tok_off;   // [n_docs + 1]
    int64_t n_docs;
    int layout;               // TD_ROWS_CONCAT / TD_ROWS_PAD
    int drop_last;            // CONCAT: the partial last row is dropped
    int64_t S;                // seq_len
    unsigned long long s_magic; // floor((2^64 - 1) / S): x / S without a 64-bit division (div_magic)
    int32_t bos, eos, pad;
    int b, e;                 // bos / eos present
    int funnel_src;           // 1: misaligned sources read as two aligned int4 and a funnel instead of four dwords (A/B)
    int32_t* out;             // [rows_cap * S]
    int64_t rows_cap;
    int32_t* pos;             // [rows_cap * S] or null
    int32_t* aux;             // CONCAT: cu_seqlens [aux_cap]; PAD: lengths [n_docs]; or null
    int64_t aux_cap;
    long long* counts;        // [4] rows, real slots, segments, truncated documents (zeroed before the launch)
    unsigned long long* scan; // cu_seqlens scan: [0] chunk ticket, [1 + c] chunk c's status (zeroed before the launch)
    int* err;
    long long* err_pos;
};

// What the host fills and the launchers take: RowsArgs, and behind it the label stream of the pair form (lab.src null: one stream).
// The one-stream kernels get the RowsArgs slice alone, so that their arguments are what they were without the pair form.
struct RowsLabArgs : RowsArgs {
    LabArgs lab;
};

// The slot kernel of the layout; behind it (CONCAT, aux set) the single-pass cu_seqlens scan.  The caller zeroes counts and
// (aux set) scan[0, rows_scan_words(n_docs)) on the same stream first.
hipError_t launch_rows(const RowsLabArgs& a, hipStream_t stream);
int64_t rows_scan_words(int64_t n_docs);

}  // namespace td
