// Decode rows (td_decode_rows.hip): what the kernels, the host library and the CPU model (tests/twin/decode_rows_model.cpp) share:
// the kernels' arguments, the per-id table's entry, the aggregate of a run of positions and its operator.  The rule is the contract
// in include/tokendagger_hip.h (td_decode_spec).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace td {

constexpr int DCR_THREADS = 256;   // lanes of a workgroup of td_dcr_sum and td_dcr_scan (td_rows_common.h's RC_THREADS); td_dcr_emit takes 512
constexpr int DCR_TILE = 4096;     // positions a workgroup takes per tile, sixteen (td_dcr_emit: eight) consecutive ones a lane (RC_TILE)
constexpr int DCR_WIN = 32768;     // bytes of the LDS window a tile's bytes leave through (the last 16 are the alignment shift's)
constexpr int DCR_MARK_IDS = 192;  // listed ids one launch of td_dcr_mark carries in its arguments

// The per-id table, one word per id in [0, max_id]: the token's byte length (0: no token, or nothing to emit), and two bits.
// An id that stops its segment and is not kept is marked skipped as well, so a kernel asks: stop? then skip? then length.
constexpr uint32_t DCR_STOP = 1u << 31;  // the id stops its segment
constexpr uint32_t DCR_SKIP = 1u << 30;  // the id emits nothing and is no error
constexpr uint32_t DCR_LEN = DCR_SKIP - 1;
constexpr uint32_t DCR_BAD = 0;          // the entry of an id that is no token and is not listed

// What a run of consecutive positions does to the byte count, whatever happened in front of it.
//   f    a segment starts inside the run
//   a    live bytes in front of the first start (of the whole run without one), GIVEN that the segment that enters the run is open
//   b    live bytes from the first start on
//   st   the run's last segment (the entering one without a start) has met a stop id inside the run, behind its start
// One position: {start, start ? 0 : bytes, start ? bytes : 0, stop}; a position behind its row's length (rows form): {start, 0, 0, 0}.
// Associative: (x . y) . z == x . (y . z); dcr_identity() on either side changes nothing.  Not commutative.
struct DcrAgg {
    unsigned long long a, b;
    uint32_t f, st;
};
__host__ __device__ inline DcrAgg dcr_identity() { return DcrAgg{0, 0, 0, 0}; }
__host__ __device__ inline DcrAgg dcr_op(const DcrAgg& x, const DcrAgg& y) {  // x in front of y
    DcrAgg r;
    const unsigned long long ya = x.st ? 0ull : y.a;  // y's entering segment is x's last one
    r.f = x.f | y.f;
    r.a = x.f ? x.a : x.a + ya;
    r.b = x.f ? x.b + ya + y.b : y.b;
    r.st = y.f ? y.st : (x.st | y.st);
    return r;
}
// a run entered in state `stopped`: its bytes, and the state it leaves
__host__ __device__ inline unsigned long long dcr_bytes(const DcrAgg& x, bool stopped) { return (stopped ? 0ull : x.a) + x.b; }
__host__ __device__ inline bool dcr_leaves_stopped(const DcrAgg& x, bool stopped) { return x.f ? x.st != 0 : (stopped || x.st != 0); }

// A tile's base in the scan's output: the bytes in front of it, and in the top bit whether its entering segment has stopped.
constexpr unsigned long long DCR_BASE_STOPPED = 1ull << 63;

// info[4]
enum { DCR_I_BYTES = 0, DCR_I_EMITTED = 1, DCR_I_SKIPPED = 2, DCR_I_STOPPED = 3 };

struct DcrHi {  // a listed id above max_id: bits = DCR_STOP | DCR_SKIP
    int32_t id;
    uint32_t bits;
};

struct DecodeRowsArgs {
    const int32_t* ids;        // [n_tokens]; no id at or above n_tokens is read
    int64_t n_tokens;
    const int64_t* tok_off;    // offsets form: [n_segs + 1]
    const int32_t* seg_len;    // rows form: [n_segs] or null (every row is row_stride long)
    int64_t n_segs;
    int64_t row_stride;        // 0: offsets form
    unsigned long long stride_magic;  // rows form: floor((2^64 - 1) / row_stride)
    const uint32_t* table;     // [max_id + 1]
    const DcrHi* hi;           // [n_hi] listed ids above max_id
    int32_t n_hi;
    int32_t max_id;
    int32_t skip_negative;
    int32_t n_tiles;           // tiles of the visited positions (the grid of td_dcr_sum and td_dcr_emit)
    const uint32_t* src_off;   // Tables::tok_off [max_id + 2]
    const uint8_t* src_bytes;  // Tables::tok_bytes
    DcrAgg* agg;               // [n_tiles]
    unsigned long long* base;  // [n_tiles + 1]: the tiles' bases, the total behind them
    uint8_t* out;
    int64_t out_cap;
    long long* out_offsets;    // [n_segs + 1]
    long long* seg_ids;        // [n_segs] or null
    unsigned long long* info;  // [4], zeroed before the launches
    int* err;
    long long* err_pos;
};

struct DcrMarkArgs {  // td_dcr_mark: n listed ids (unique over a call's launches) and their bits; those above max_id go to hi[hi_at[i]]
    uint32_t* table;
    DcrHi* hi;
    int32_t max_id;
    int32_t n;
    int32_t ids[DCR_MARK_IDS];
    uint16_t hi_at[DCR_MARK_IDS];
    uint8_t bits[DCR_MARK_IDS];  // 1 = skip, 2 = stop
};
constexpr int DCR_MAX_HI = 65535;  // listed ids above max_id at most (DcrMarkArgs::hi_at)

// the tiles of a call whose positions end at `end` (n_tokens, or n_segs * row_stride): absolute multiples of DCR_TILE from 0 on; a
// tile in front of tok_off[0] costs a workgroup that leaves at once
inline int64_t dcr_tiles(int64_t end) { return (end + DCR_TILE - 1) / DCR_TILE; }

hipError_t launch_decode_rows_table(uint32_t* table, const uint32_t* tok_off, int32_t max_id, hipStream_t stream);
hipError_t launch_decode_rows_mark(const DcrMarkArgs& m, hipStream_t stream);
// plain: no id is listed, no flag is set (the table holds lengths only and nothing stops).  phases: 1 = td_dcr_sum + td_dcr_scan
// (the total, TD_E_CAPACITY and out_offsets[n_segs] are known behind them), 2 = td_dcr_emit, 3 = all three.
hipError_t launch_decode_rows(const DecodeRowsArgs& a, bool plain, int phases, hipStream_t stream);

}  // namespace td
