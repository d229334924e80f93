// Token counts (td_counts.hip): what the kernel, the host library and the CPU model (tests/twin/counts_model.cpp) share: the
// kernel's arguments, its constants and the seat hash.  The rule is the contract in include/tokendagger_hip.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace td {

constexpr int CNT_THREADS = 256;      // lanes of a workgroup (td_rows_common.h's RC_THREADS)
constexpr int CNT_TILE = 4096;        // ids a workgroup counts per tile, four int4 loads a lane (RC_TILE)
constexpr int CNT_MAX_GRID = 1024;    // workgroups at most (RC_MAX_GRID / 2: every workgroup ends with a flush of its table)
constexpr int CNT_MIN_TILES = 8;      // a call's grid gives every workgroup at least this many tiles (when it has them): small calls flush few tables
constexpr int CNT_SEATS = 4096;       // seats of a workgroup's on-chip table, the production size: 8 B a seat, 32 KiB of LDS
constexpr int CNT_FLUSH_TILES = 64;   // the table is flushed and cleared behind every this many tiles of a workgroup: a 32-bit seat
                                      // counter holds at most CNT_FLUSH_TILES * CNT_TILE = 2^18 < 2^31
constexpr int32_t CNT_EMPTY = -1;     // a seat nobody has taken (keys are 0 .. 2^28 - 1)
constexpr int64_t CNT_MAX_KEYS = 1ll << 28;  // n_groups * n_bins at most
static_assert((int64_t)CNT_FLUSH_TILES * CNT_TILE < (1ll << 31), "a seat's counter between two flushes");
static_assert((CNT_SEATS & (CNT_SEATS - 1)) == 0 && CNT_TILE == 16 * CNT_THREADS, "seats: a power of two; sixteen ids a lane");

// CountsArgs::info
enum { CNT_I_COUNTED = 0, CNT_I_NEGATIVE = 1, CNT_I_TOO_LARGE = 2, CNT_I_BAD_GROUP = 3 };

// The first seat key `key` tries, of 2^seat_bits (1 <= seat_bits <= 12); the second and last is that seat ^ 1.  Fibonacci hashing:
// the ids that occur together are neither consecutive nor spread evenly, the product's top bits mix all of the key's.
__host__ __device__ inline uint32_t cnt_seat(int32_t key, int seat_bits) { return ((uint32_t)key * 0x9E3779B1u) >> (32 - seat_bits); }

// the grid of a call on n_tokens ids
inline int cnt_grid(int64_t n_tokens) {
    const int64_t tiles = (n_tokens + CNT_TILE - 1) / CNT_TILE;
    const int64_t g = (tiles + CNT_MIN_TILES - 1) / CNT_MIN_TILES;
    return (int)(g < 1 ? 1 : g > CNT_MAX_GRID ? CNT_MAX_GRID : g);
}

struct CountsArgs {
    const int32_t* ids;        // [n_tokens]
    int64_t n_tokens;          // no id at or above it is read
    const int64_t* tok_off;    // [n_docs + 1] with doc_group; null without it: positions [0, n_tokens) are visited
    int64_t n_docs;
    const int32_t* doc_group;  // [n_docs], or null: one group, tok_off and n_docs are not looked at
    int64_t n_bins;
    int64_t n_groups;
    int32_t seat_bits;         // the table has 2^seat_bits seats
    int32_t flush_tiles;       // 1 .. CNT_FLUSH_TILES: the default, or less (TD_OPT_COUNTS_FLUSH_TILES; the model shrinks it too)
    unsigned long long* counts;  // [n_groups * n_bins], zeroed or accumulated into
    unsigned long long* info;    // [4], zeroed before the launch
    int* err;
    long long* err_pos;
};

}  // namespace td
