// Per-token start offsets (td_offsets.hip): where in its document every token's text begins, in bytes or in code points.
// Kept apart from EncodeArgs / Tables: the per-id character table below is an argument of these kernels only (the fused tile
// loop's argument and table footprint is tuned).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace td {

constexpr int OFF_CHUNK = 4096;  // ids per chunk of the segmented scan (one workgroup of 1024 lanes, four ids a lane)
constexpr int OFF_TILE = 4096;   // text bytes per tile of the rank / select structures (128 bitmap words)
enum OffKind : int {
    OFF_BYTES = 0,  // the scan sums token byte lengths
    OFF_CHARS = 1,  // ... character counts; the start is max(0, sum - first byte is a continuation byte)
    OFF_PAIR = 2,   // ... both, packed chars << 32 | bytes (a document below 4 GiB), unpacked by td_off_finish
};

struct StartsArgs {
    const int32_t* tokens;          // ids
    const int64_t* tok_off;         // [n_docs + 1] first id of every document
    int64_t n_docs;
    int64_t n_bound;                // ids the arrays hold: ids at or behind min(tok_off[n_docs], n_bound) are not read
    const uint32_t* len_off;        // Tables::tok_off: the bytes of id k are [len_off[k], len_off[k + 1])
    const uint32_t* ctab;           // id -> char_count << 1 | first byte is a continuation byte; 0: not a token
    int32_t max_id;
    int kind;                       // OffKind
    int64_t* out;                   // [n_bound] starts
    uint32_t* heads;                // [n_bound / 32 + 2] bit i: id i is the first of a document
    unsigned long long* chunk_sum;  // [chunks + 1] chunk totals, then the carry into every chunk
    uint32_t* chunk_head;           // [chunks + 1] the chunk holds a document start
    int* err;
    long long* err_pos;
    // encode only (launch_encode_starts, launch_chars_by_rank)
    const uint8_t* text;
    int64_t n;
    const int64_t* doc_off;         // [n_docs + 1] byte offsets of the documents
    uint8_t* doc_gap;               // [n_docs] 1: the document's ids cover fewer bytes than it has
    int generic;                    // the pattern may skip text; otherwise a document that is not covered exactly is an error
    int chars;                      // the result is in code points
    const uint32_t* startbits;      // the generic engine's piece-start and skipped-stretch bitmaps of the same call
    const uint32_t* gapbits;
    uint32_t* covbits;              // [words + 1] bit p: byte p is covered by a token
    uint32_t* ncbits;               // [words + 1] bit p: byte p is not a continuation byte
    uint16_t* cov_wpref;            // [words + 1] covered bytes in front of the word inside its tile
    uint16_t* nc_wpref;
    int64_t* cov_tpref;             // [tiles + 1] covered bytes in front of the tile
    int64_t* nc_tpref;
    uint32_t* tile_kind;            // [tiles + 1] last piece start of the tile (1 piece, 2 skipped, 0 none), then the kind in force at its start
};

// td_token_starts: the covered rule on ids alone (heads, chunk scan, chunk carries, starts)
hipError_t launch_token_starts(const StartsArgs& a, hipStream_t stream);
// its middle alone, on a.heads already filled: the chunk totals, then in their place the carry into every chunk (a.chunk_sum[c] =
// the bytes of chunk c's first document in front of the chunk; ids that are no tokens raise TD_E_BAD_TOKEN).  a.out is not touched.
hipError_t launch_chunk_carries(const StartsArgs& a, hipStream_t stream);
// behind launch_token_starts inside an encode: every document checked against its byte length; for generic patterns the
// documents with skipped text mapped to source positions; OFF_PAIR unpacked
hipError_t launch_encode_starts(const StartsArgs& a, hipStream_t stream);
// out holds document-relative BYTE starts of every document: into code points by rank over the text
hipError_t launch_chars_by_rank(const StartsArgs& a, hipStream_t stream);
// scratch sizes (bytes) of the rank structures for n bytes of text, carved by off_rank_layout
size_t off_rank_bytes(int64_t n);
void off_rank_layout(StartsArgs& a, void* base, int64_t n);

}  // namespace td
