// The text rewrites (td_nfc.hip, td_utf8.hip): what the two passes' arguments, constants and host statements have in common.  A rewrite
// checks documents at read speed, measures its output a tile, scans the tiles' sizes and writes (td_rewrite_common.h has the kernels'
// frame); its arguments are RewriteArgs plus what the pass adds (NfcArgs, U8Args).  Compiles on the host without HIP's runtime
// (tools/sanitize/utf8_asan.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace td {

constexpr int RW_THREADS = 256;              // lanes of a workgroup (RC_THREADS)
constexpr int RW_TILE = RW_THREADS * 16;     // bytes of a workgroup's tile: a window of 16 bytes a lane

// launch_nfc / launch_utf8: the phases of a call (a host form sizes the output from counts[0] between the two)
enum { RW_RUN_MEASURE = 1, RW_RUN_WRITE = 2 };
// counts[8]: the output's bytes first, the rest is the pass's
enum { RW_C_BYTES = 0, RW_C_WORDS = 8 };
// RewriteArgs::head, zeroed before the launches: 2^62 - the lowest document with bad offsets (0: none), kept by an atomic maximum; 1 when
// the output does not fit
enum { RW_H_BAD = 0, RW_H_FULL = 1, RW_H_WORDS = 4 };
// what a lane's walk over its window does: sizes and the per-document results, sizes alone, the bytes
enum { RW_MEASURE = 0, RW_SIZE = 1, RW_WRITE = 2 };

struct RewriteArgs {
    const uint8_t* text;       // [n_bytes]
    int64_t n_bytes;
    const int64_t* doc_off;    // [n_docs + 1]
    int64_t n_docs;
    uint8_t* flags;            // [n_docs]
    uint8_t* out;              // [out_capacity]
    int64_t out_capacity;
    int64_t* out_doc_off;      // [n_docs + 1]
    unsigned long long* counts;     // [RW_C_WORDS]
    unsigned long long* tile_base;  // [tiles + 1]: the tiles' output bytes, then their exclusive prefixes
    unsigned long long* head;       // [RW_H_WORDS]
    int* err;
    long long* err_pos;
};

inline bool rewrite_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// offsets from 0, non-decreasing (what every host statement checks first)
inline bool rewrite_offsets_ok(const int64_t* off, int64_t n_docs) {
    if (off[0] != 0) return false;
    for (int64_t d = 0; d < n_docs; ++d)
        if (off[d + 1] < off[d]) return false;
    return true;
}

}  // namespace td
