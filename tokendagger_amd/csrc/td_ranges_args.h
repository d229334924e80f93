// Loss labels from byte ranges (td_ranges.hip): the kernels' arguments and their launch, for the host library.  The rule is the
// contract in include/tokendagger_hip.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_labels_args.h"
#include "td_offsets.h"

namespace td {

constexpr int RNG_TILE = LAB_TILE;  // ids a workgroup labels per tile, sixteen a lane: td_lab_finish reads what td_rng_apply leaves
constexpr int RNG_WIN = 512;        // ranges of a tile's window kept in LDS (begin, end, marked bytes in front: 24 B each); more: global memory
constexpr int RNG_CHUNK = 1024;     // ranges per workgroup of td_rng_check, four a lane
static_assert(RNG_TILE == OFF_CHUNK, "a tile's carry is td_off_carry's chunk carry");
// RangeArgs::head: LabelArgs::head's words (LAB_H_BAD; LAB_H_TRAINED, LAB_H_SPANS = partially marked ids, LAB_H_UNTERM = marked
// bytes; LAB_H_END stays 0), then as 2^63 - 1 - index, 0 = none (the lowest index wins): the first range out of order, the first
// range that ends behind its document's bytes, the first document whose ids do not cover its text
enum { RNG_H_RANGE = 5, RNG_H_BEYOND = 6, RNG_H_GAP = 7 };
static_assert(LAB_HEAD_WORDS == 8 && LAB_H_END == 4, "RangeArgs::head");

struct RangeArgs {
    const int32_t* ids;            // [n_tokens]
    int64_t n_tokens;              // ids the buffer holds: tok_off[n_docs] above it is an error, no id at or above it is read
    const int64_t* tok_off;        // [n_docs + 1]
    int64_t n_docs;
    const int64_t* starts;         // [n_tokens] byte starts, or null: scanned from the lengths (the covered rule)
    const int64_t* range_off;      // [n_docs + 1]
    const long long* ranges;       // [n_ranges][2] begin, end
    int64_t n_ranges;
    int32_t rule;                  // TD_RANGE_*
    int32_t ignore;
    const uint32_t* len_off;       // Tables::tok_off: the bytes of id k are [len_off[k], len_off[k + 1])
    int32_t max_id;
    const int64_t* doc_off;        // covered form, or null: [n_docs + 1] byte offsets of the documents' text, every document's ids must cover it
    int32_t* labels;               // [n_tokens]
    uint8_t* mask;                 // [n_tokens] or null
    int64_t* trained_off;          // [n_docs + 1] or null
    long long* counts;             // [4] trained ids, partially marked ids, marked bytes, 0
    // workspace
    unsigned long long* head;      // [LAB_HEAD_WORDS], zeroed before the launch
    uint32_t* bits;                // [n_tokens / 32 + 2], zeroed: a non-empty document starts at this id (td_off_heads' form)
    uint32_t* rbits;               // [n_ranges / 32 + 2], zeroed: a document's first range
    long long* cum;                // [n_ranges]: the marked bytes in front of range r inside its chunk of RNG_CHUNK ranges
    unsigned long long* rchunks;   // [n_ranges / RNG_CHUNK + 2]: a chunk's marked bytes, then those in front of the chunk
    unsigned long long* chunk_sum; // covered form: [n_tokens / OFF_CHUNK + 2] and behind them as many uint32 (StartsArgs::chunk_sum, chunk_head)
    unsigned long long* tile_cnt;  // (trained_off only) as LabelArgs
    uint32_t* aux;                 // (trained_off only) as LabelArgs
    int* err;
    long long* err_pos;
};

// td_rng_docs, td_rng_check, td_rng_cum, [launch_chunk_carries,] td_rng_apply, [td_rng_status,] launch_labels_finish
hipError_t launch_range_labels(const RangeArgs& a, hipStream_t stream);

}  // namespace td
