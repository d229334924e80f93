// CPU model of td_decode_rows.hip's decomposition, over the shared header (tokendagger_amd/csrc/td_decode_rows_args.h: the table's
// entry, the aggregate and its operator).  The tile size is a parameter.  What it follows from the kernels:
//
//   table    td_dcr_table / td_dcr_mark: lengths, then the distinct listed ids with their bits; those above max_id in a list
//   sum      per tile of absolute multiples of `tile`: every visited position as ONE aggregate, folded with dcr_op
//   scan     the tiles' aggregates to each tile's byte base and entering state, the total, TD_E_CAPACITY
//   emit     per tile, from the entering state: the walk (errors, seg_ids where a segment stops or ends, byte prefixes at the starts),
//            out_offsets of the segments whose offset lies in the tile (the last tile takes those at its end), the bytes
// The kernel folds sixteen positions a lane and scans lanes and wavefronts; the operator is associative, so the order of the folding
// does not matter and the model folds position by position.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tokendagger_amd/csrc/td_decode_rows_args.h"

using namespace td;

namespace {

constexpr int E_INVALID = 1, E_CAPACITY = 5, E_BAD_TOKEN = 8;

struct Model {
    const int32_t* ids; int64_t n_tokens; const int64_t* tok_off; const int32_t* seg_len; int64_t n_segs, stride;
    std::vector<uint32_t> table; std::vector<DcrHi> hi; int32_t max_id; bool skip_negative;
    const uint32_t* src_off; const uint8_t* src_bytes;
    uint8_t* out; int64_t out_cap; int64_t* out_offsets; int64_t* seg_ids; int64_t* info;
    int64_t tile;
    int err = 0; int64_t err_pos = -1;

    void raise(int code, int64_t pos) {
        if (code == E_BAD_TOKEN) {  // the lowest index wins, while the error on record is this one
            if (!err || err == E_BAD_TOKEN) { err_pos = err ? (pos < err_pos ? pos : err_pos) : pos; err = code; }
        } else if (!err) { err = code; err_pos = pos; }
    }
    uint32_t entry(int32_t id) const {
        if (id >= 0 && id <= max_id) return table[(size_t)id];
        if (id < 0) return skip_negative ? DCR_SKIP : DCR_BAD;
        for (const DcrHi& h : hi) if (h.id == id) return h.bits;
        return DCR_BAD;
    }
    int64_t row_len(int64_t r, bool rs) {
        if (!seg_len) return stride;
        const int64_t n = seg_len[r];
        if (n < 0 || n > stride) { if (rs) raise(E_INVALID, r); return n < 0 ? 0 : stride; }
        return n;
    }
    // position p: does a segment start there, is it behind its row's length
    void place(int64_t p, const std::vector<uint8_t>& start_at, int64_t lo, bool& start, bool& dead, bool rs) {
        if (stride) {
            const int64_t r = p / stride, q = p - r * stride;
            start = q == 0;
            dead = q >= row_len(r, rs);
        } else {
            start = start_at[(size_t)(p - lo)] != 0;
            dead = false;
        }
    }

    void run() {
        int64_t lo = 0, hi_ = n_segs * stride;
        if (!stride) {
            lo = tok_off[0]; hi_ = tok_off[n_segs];
            if (lo < 0 || hi_ < lo || hi_ > n_tokens) {
                raise(E_INVALID, lo < 0 ? 0 : n_segs);
                lo = lo < 0 ? 0 : lo; hi_ = hi_ > n_tokens ? n_tokens : hi_; hi_ = hi_ < lo ? lo : hi_;
            }
            for (int64_t d = 0; d < n_segs; ++d) if (tok_off[d + 1] < tok_off[d]) raise(E_INVALID, d);
        }
        const int64_t hi = hi_;
        std::vector<uint8_t> start_at((size_t)(hi - lo + 1), 0);
        if (!stride) for (int64_t d = 0; d <= n_segs; ++d) if (tok_off[d] >= lo && tok_off[d] <= hi) start_at[(size_t)(tok_off[d] - lo)] = 1;
        const int64_t n_tiles = ((stride ? hi : n_tokens) + tile - 1) / tile;
        // sum
        std::vector<DcrAgg> agg((size_t)n_tiles, dcr_identity());
        for (int64_t t = 0; t < n_tiles; ++t) {
            const int64_t s0 = t * tile > lo ? t * tile : lo, s1 = (t + 1) * tile < hi ? (t + 1) * tile : hi;
            DcrAgg g = dcr_identity();
            bool looked = true;  // (an id behind its segment's stop is not looked at: the fold knows when)
            for (int64_t p = s0; p < s1; ++p) {
                bool start, dead;
                place(p, start_at, lo, start, dead, false);
                DcrAgg one{0, 0, start ? 1u : 0u, 0};
                if (start) looked = true;
                if (!dead && looked) {
                    const uint32_t e = entry(ids[p]);
                    (start ? one.b : one.a) = e & DCR_LEN;
                    one.st = e >> 31;
                    if (one.st) looked = false;
                }
                g = dcr_op(g, one);
            }
            agg[(size_t)t] = g;
        }
        // scan
        std::vector<unsigned long long> base((size_t)n_tiles + 1);
        DcrAgg run = dcr_identity();
        for (int64_t t = 0; t < n_tiles; ++t) {
            base[(size_t)t] = dcr_bytes(run, false) | (dcr_leaves_stopped(run, false) ? DCR_BASE_STOPPED : 0ull);
            run = dcr_op(run, agg[(size_t)t]);
        }
        const int64_t total = (int64_t)dcr_bytes(run, false);
        base[(size_t)n_tiles] = (unsigned long long)total;
        out_offsets[n_segs] = total;
        info[DCR_I_BYTES] = total;
        if (total > out_cap) raise(E_CAPACITY, total);
        if (lo >= hi) for (int64_t d = 0; d < n_segs; ++d) { out_offsets[d] = 0; if (seg_ids) seg_ids[d] = 0; }
        // emit
        for (int64_t t = 0; t < n_tiles; ++t) {
            const int64_t s0 = t * tile > lo ? t * tile : lo, s1 = (t + 1) * tile < hi ? (t + 1) * tile : hi;
            if (s0 >= s1) continue;
            bool stopped = (base[(size_t)t] & DCR_BASE_STOPPED) != 0;
            int64_t at = (int64_t)(base[(size_t)t] & ~DCR_BASE_STOPPED);
            std::vector<int64_t> pre((size_t)(s1 - s0 + 1), -1);
            for (int64_t p = s0; p < s1; ++p) {
                bool start, dead;
                place(p, start_at, lo, start, dead, true);
                bool last;
                if (stride) {
                    const int64_t r = p / stride, q = p - r * stride, n = row_len(r, false);
                    last = q + 1 == n;
                    if (start) { out_offsets[r] = at; if (n == 0 && seg_ids) seg_ids[r] = 0; }
                } else {
                    last = p + 1 == hi || start_at[(size_t)(p + 1 - lo)];
                    if (start) pre[(size_t)(p - s0)] = at;
                }
                if (start) stopped = false;
                if (dead || stopped) continue;
                const uint32_t e = entry(ids[p]);
                const uint32_t len = e & DCR_LEN;
                if (len) {
                    ++info[DCR_I_EMITTED];
                    if (total <= out_cap && out) memcpy(out + at, src_bytes + src_off[ids[p]], len);
                    at += len;
                } else if (e & DCR_SKIP) ++info[DCR_I_SKIPPED];
                else raise(E_BAD_TOKEN, p);
                if (e >> 31) { stopped = true; ++info[DCR_I_STOPPED]; }
                if (seg_ids && ((e >> 31) || last)) {
                    if (stride) seg_ids[p / stride] = p % stride + 1;
                    else {
                        int64_t a = 0, b = n_segs;  // the last segment whose offset is <= p
                        while (b - a > 1) { const int64_t m = a + (b - a) / 2; if (tok_off[m] <= p) a = m; else b = m; }
                        if (tok_off[a] <= p) seg_ids[a] = p + 1 - tok_off[a];
                    }
                }
            }
            if (!stride) {
                pre[(size_t)(s1 - s0)] = at;
                for (int64_t d = 0; d <= n_segs; ++d) {
                    const int64_t p = tok_off[d];
                    if (p < s0 || p > s1 || (p == s1 && s1 != hi)) continue;
                    out_offsets[d] = pre[(size_t)(p - s0)];
                    if (seg_ids && d < n_segs && tok_off[d + 1] == p) seg_ids[d] = 0;
                }
            }
        }
    }
};

}  // namespace

extern "C" {

// lens[max_id + 1]: the tokens' byte lengths (0: no token); listed[n_listed] distinct ids with bits[n_listed] (1 = skip, 2 = stop).
// src_off[max_id + 2], src_bytes: the tokens' bytes.  Returns the error code, *err_pos its position.
int decode_rows_model(const int32_t* ids, int64_t n_tokens, const int64_t* tok_off, const int32_t* seg_len, int64_t n_segs, int64_t stride,
                      const uint32_t* lens, int32_t max_id, const int32_t* listed, const uint8_t* bits, int64_t n_listed, int skip_negative,
                      const uint32_t* src_off, const uint8_t* src_bytes, int64_t tile, uint8_t* out, int64_t out_cap, int64_t* out_offsets,
                      int64_t* seg_ids, int64_t* info, int64_t* err_pos) {
    Model m;
    m.ids = ids; m.n_tokens = n_tokens; m.tok_off = tok_off; m.seg_len = seg_len; m.n_segs = n_segs; m.stride = stride;
    m.max_id = max_id; m.skip_negative = skip_negative != 0; m.src_off = src_off; m.src_bytes = src_bytes;
    m.out = out; m.out_cap = out_cap; m.out_offsets = out_offsets; m.seg_ids = seg_ids; m.info = info; m.tile = tile;
    for (int32_t id = 0; id <= max_id; ++id) m.table.push_back(lens[id] & DCR_LEN);
    for (int64_t i = 0; i < n_listed; ++i) {  // td_dcr_mark
        const uint32_t b = ((bits[i] & 1) ? DCR_SKIP : 0u) | ((bits[i] & 2) ? DCR_STOP : 0u);
        if (listed[i] <= max_id) m.table[(size_t)listed[i]] = ((b & DCR_SKIP) ? 0u : (m.table[(size_t)listed[i]] & DCR_LEN)) | b;
        else m.hi.push_back(DcrHi{listed[i], b});
    }
    for (int k = 0; k < 4; ++k) info[k] = 0;
    m.run();
    *err_pos = m.err_pos;
    return m.err;
}

// x, y, out: n aggregates as (a, b, f, st) int64 quadruples; out[i] = dcr_op(x[i], y[i])
void decode_rows_model_op(int64_t n, const int64_t* x, const int64_t* y, int64_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const DcrAgg r = dcr_op(DcrAgg{(unsigned long long)x[4 * i], (unsigned long long)x[4 * i + 1], (uint32_t)x[4 * i + 2], (uint32_t)x[4 * i + 3]},
                                DcrAgg{(unsigned long long)y[4 * i], (unsigned long long)y[4 * i + 1], (uint32_t)y[4 * i + 2], (uint32_t)y[4 * i + 3]});
        out[4 * i] = (int64_t)r.a; out[4 * i + 1] = (int64_t)r.b; out[4 * i + 2] = r.f; out[4 * i + 3] = r.st;
    }
}

int64_t decode_rows_model_const(int what) {
    switch (what) {
        case 0: return DCR_TILE;
        case 1: return DCR_THREADS;
        case 2: return DCR_WIN;
        case 3: return DCR_MARK_IDS;
    }
    return -1;
}

}  // extern "C"
