// Allowed special tokens: cut out on the device (td_special.hip) or on the host, the ordinary text between them encoded as one batch.
#include "td_handle.h"
#include "td_offsets.h"
#include "td_regex.h"
#include "td_special_table.h"

namespace {

// The allowed literals (every special string that carries one of the ids) as td_special.hip wants them: sorted bytewise, each
// with the longest other literal that is a proper prefix of it, and the bitmap of their first two bytes.
int build_special_table(td_tokenizer* t, const int32_t* allowed_ids, int64_t n_allowed) {
    std::vector<int32_t> key(allowed_ids, allowed_ids + n_allowed);
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    if (key == t->sp_key && t->sp_n) return TD_OK;
    const HostTables& H = t->H;
    std::vector<std::pair<std::string, int32_t>> lits;
    for (int32_t id : key) {
        bool found = false;
        for (size_t k = 0; k < H.special_ids.size(); ++k)
            if (H.special_ids[k] == id && !H.special_strs[k].empty()) { lits.emplace_back(H.special_strs[k], id); found = true; }
        if (!found) { t->err = "Special token id " + std::to_string(id) + " not found in special encoder"; return TD_E_SPECIAL; }
    }
    std::sort(lits.begin(), lits.end(), [](const auto& x, const auto& y) { return x.first < y.first; });  // (bytewise: std::string compares as unsigned char)
    lits.erase(std::unique(lits.begin(), lits.end(), [](const auto& x, const auto& y) { return x.first == y.first; }), lits.end());
    for (const auto& lit : lits) {
        const std::string& x = lit.first;
        if (x.size() > SP_MAXLEN) {
            t->err = "td_encode_device_with_special: the allowed special token '" + x + "' is " + std::to_string(x.size()) +
                     " bytes long; the device search takes literals of at most 48 bytes (td_encode_batch_with_special searches on the host)";
            return TD_E_INVALID;
        }
    }
    const size_t n = lits.size();
    const SpecialTableHost T = special_table_build(lits);
    int rc;
    if ((rc = ensure(t, t->sp_bytes, T.bytes.size() + 16))) return rc;
    if ((rc = ensure(t, t->sp_off, (n + 1) * 4))) return rc;
    if ((rc = ensure(t, t->sp_len, (n + 1) * 4))) return rc;
    if ((rc = ensure(t, t->sp_id, std::max<size_t>(n, 1) * 4))) return rc;
    if ((rc = ensure(t, t->sp_parent, std::max<size_t>(n, 1) * 4))) return rc;
    if ((rc = ensure(t, t->sp_first2, SP_FIRST2_WORDS * 4))) return rc;
    if ((rc = own_streams(t))) return rc;
    // (the callers have waited for the kernels that read the previous table; the call that uses this one is ordered behind
    // these copies by the host: each is waited for)
    if ((rc = copy_wait(t, t->sp_bytes.p, T.bytes.data(), T.bytes.size(), hipMemcpyHostToDevice, t->s_own))) return rc;
    if ((rc = copy_wait(t, t->sp_off.p, T.off.data(), (n + 1) * 4, hipMemcpyHostToDevice, t->s_own))) return rc;
    if ((rc = copy_wait(t, t->sp_len.p, T.len.data(), (n + 1) * 4, hipMemcpyHostToDevice, t->s_own))) return rc;
    if ((rc = copy_wait(t, t->sp_id.p, T.id.data(), n * 4, hipMemcpyHostToDevice, t->s_own))) return rc;
    if ((rc = copy_wait(t, t->sp_parent.p, T.parent.data(), n * 4, hipMemcpyHostToDevice, t->s_own))) return rc;
    if ((rc = copy_wait(t, t->sp_first2.p, T.first2.data(), SP_FIRST2_WORDS * 4, hipMemcpyHostToDevice, t->s_own))) return rc;
    t->sp_key = key;
    t->sp_n = (uint32_t)n;
    t->sp_maxlen = T.maxlen;
    return TD_OK;
}

// What the device search needs before its encode_device_locked: the table of this allowed set (the previous call's may still be
// read by its kernels: a different set waits for them) and the hit, accept and candidate buffers for n bytes of text.
int special_search_prepare(td_tokenizer* t, const int32_t* allowed_ids, int64_t n_allowed, int64_t n) {
    std::vector<int32_t> key(allowed_ids, allowed_ids + n_allowed);
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    if (key != t->sp_key && t->has_last) HIP_TRY(t, hipEventSynchronize(t->last_done));
    int rc;
    if ((rc = build_special_table(t, allowed_ids, n_allowed))) return rc;
    if ((rc = ensure(t, t->sp_hit, (size_t)((n + 31) / 32 + 8) * 4))) return rc;
    if ((rc = ensure(t, t->sp_acc, (size_t)((n + 31) / 32 + 8) * 4))) return rc;
    if ((rc = ensure(t, t->sp_cpos, (size_t)(n / 32 + 4096) * 8))) return rc;   // candidates: room for one per 32 bytes
    if ((rc = ensure(t, t->sp_clit, (size_t)(n / 32 + 4096) * 4))) return rc;
    return ensure(t, t->sp_ccount, 64);
}

// Allowed special tokens indexed by their first two bytes: one pass over the text finds, at every position, the
// longest allowed special that starts there (tiktoken semantics: cut at the EARLIEST occurrence; longest on ties).
struct SpecialIndex {
    struct Ent { const std::string* s; int32_t id; };
    bool first[256] = {};
    std::vector<Ent> ents;       // sorted by (first byte, second byte or -1, longer first)
    uint32_t lo[257] = {};       // ents[lo[b0] .. lo[b0 + 1]): the literals that start with byte b0
    size_t count = 0;
    static int second(const std::string& x) { return x.size() > 1 ? (uint8_t)x[1] : -1; }
    void add(const std::string* s, int32_t id) {
        if (s->empty()) return;
        ++count;
        ents.push_back({s, id});
    }
    void finish() {  // (cost proportional to the allowed set: nothing for an empty one)
        std::sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) {
            const uint8_t a0 = (uint8_t)(*x.s)[0], b0 = (uint8_t)(*y.s)[0];
            if (a0 != b0) return a0 < b0;
            const int a1 = second(*x.s), b1 = second(*y.s);
            if (a1 != b1) return a1 < b1;
            return x.s->size() > y.s->size();
        });
        uint32_t k = 0;
        for (int b = 0; b < 256; ++b) {
            lo[b] = k;
            while (k < ents.size() && (uint8_t)(*ents[k].s)[0] == b) ++k;
            first[b] = k > lo[b];
        }
        lo[256] = k;
    }
    // longest special starting at text[p] (p < hi), or nullptr
    const Ent* match(const uint8_t* text, int64_t p, int64_t hi) const {
        const uint8_t b0 = text[p];
        if (!first[b0]) return nullptr;
        const Ent* single = nullptr;
        const Ent* e = ents.data() + lo[b0];
        const Ent* end = ents.data() + lo[b0 + 1];
        if (e < end && e->s->size() == 1) { single = e; ++e; }  // (second byte -1 sorts first)
        if (p + 1 < hi) {
            const int b1 = text[p + 1];
            // first literal whose second byte is b1 (binary search over the literals of this first byte)
            const Ent* a = e;
            const Ent* z = end;
            while (a < z) { const Ent* m = a + (z - a) / 2; if (second(*m->s) < b1) a = m + 1; else z = m; }
            for (; a < end && second(*a->s) == b1; ++a)
                if (p + (int64_t)a->s->size() <= hi && memcmp(text + p, a->s->data(), a->s->size()) == 0) return a;
        }
        return single;
    }
};

// The allowed set arrives either as special-token STRINGS (exactly those literals are cut out, tiktoken's
// allowed_special) or as ids (every special string that carries one of the ids — two strings may share an id).
int build_special_index(td_tokenizer* t, const uint8_t* allowed_bytes, const int64_t* allowed_offsets, const int32_t* allowed_ids,
                        int64_t n_allowed, SpecialIndex& ix) {
    const HostTables& H = t->H;
    for (int64_t k = 0; k < n_allowed; ++k) {
        bool found = false;
        if (allowed_offsets) {
            const int64_t lo = allowed_offsets[k], hi = allowed_offsets[k + 1];
            if (hi < lo) { t->err = "allowed_offsets must be non-decreasing"; return TD_E_INVALID; }
            const std::string want((const char*)allowed_bytes + lo, (size_t)(hi - lo));
            for (size_t s = 0; s < H.special_strs.size(); ++s)
                if (H.special_strs[s] == want) { ix.add(&H.special_strs[s], H.special_ids[s]); found = true; break; }
            if (!found) { t->err = "Special token '" + want + "' not found in special encoder"; return TD_E_SPECIAL; }  // tiktoken.cpp:178-180
        } else {
            for (size_t s = 0; s < H.special_ids.size(); ++s)
                if (H.special_ids[s] == allowed_ids[k]) { ix.add(&H.special_strs[s], allowed_ids[k]); found = true; }
            if (!found) { t->err = "Special token id " + std::to_string(allowed_ids[k]) + " not found in special encoder"; return TD_E_SPECIAL; }
        }
    }
    ix.finish();
    return TD_OK;
}

// document text[lo, hi) -> (start, end) of its ordinary segments + the special id that follows each
void segment_document(const SpecialIndex& ix, const uint8_t* text, int64_t lo, int64_t hi, std::vector<int64_t>& starts,
                      std::vector<int64_t>& ends, std::vector<int32_t>& seg_special) {
    int64_t start = lo;
    if (ix.count)
        for (int64_t p = lo; p < hi;) {
            // memchr-speed skip to the next byte that can begin an allowed special
            const SpecialIndex::Ent* e = ix.match(text, p, hi);
            if (!e) { ++p; continue; }
            starts.push_back(start); ends.push_back(p); seg_special.push_back(e->id);
            p += (int64_t)e->s->size();
            start = p;
        }
    starts.push_back(start); ends.push_back(hi); seg_special.push_back(-1);
}

// Document-relative byte starts (host) -> characters, by rank over the documents' text on the device (td_encode_batch_with_starts
// behind allowed special tokens: segments are encoded in bytes, stitched on the host, then converted here).
int chars_by_rank_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const int64_t* tok_offsets,
                         int64_t* starts, int64_t n_tok) {
    const int64_t n = doc_offsets[n_docs];
    if (n_tok <= 0 || n <= 0) return TD_OK;
    int rc;
    if ((rc = ensure(t, t->h2d_text, (size_t)n + 64))) return rc;
    if ((rc = ensure(t, t->h2d_offs, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->d_offsets, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->off_starts, (size_t)n_tok * 8))) return rc;
    if ((rc = ensure(t, t->off_rank, off_rank_bytes(n)))) return rc;
    if ((rc = own_streams(t))) return rc;
    hipStream_t s = t->s_own;
    if ((rc = order_before(t, s))) return rc;
    HIP_TRY(t, hipMemcpyAsync(t->h2d_text.p, text, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(t, hipMemcpyAsync(t->h2d_offs.p, doc_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(t, hipMemcpyAsync(t->d_offsets.p, tok_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(t, hipMemcpyAsync(t->off_starts.p, starts, (size_t)n_tok * 8, hipMemcpyHostToDevice, s));
    StartsArgs a;
    memset(&a, 0, sizeof a);
    a.tok_off = (const int64_t*)t->d_offsets.p;
    a.n_docs = n_docs;
    a.n_bound = n_tok;
    a.out = (int64_t*)t->off_starts.p;
    a.text = (const uint8_t*)t->h2d_text.p;
    a.n = n;
    a.doc_off = (const int64_t*)t->h2d_offs.p;
    a.chars = 1;
    off_rank_layout(a, t->off_rank.p, n);
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, launch_chars_by_rank(a, s));
    if ((rc = order_after(t, s))) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    return copy_wait(t, starts, t->off_starts.p, (size_t)n_tok * 8, hipMemcpyDeviceToHost, s);
}

// Shared body of the two *_with_special entry points (handle locked by the caller).
int encode_special_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                          const uint8_t* allowed_bytes, const int64_t* allowed_offsets, const int32_t* allowed_ids, int64_t n_allowed,
                          int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens,
                          int64_t* last_seg_lo, int64_t* last_seg_hi, int unit = TD_UNIT_BYTES, int64_t* out_starts = nullptr) {
    int rc;
    if ((rc = check_offsets(t, "doc_offsets", doc_offsets, n_docs, text))) return rc;
    if (n_allowed == 0) {  // nothing to cut out: the documents are the segments
        if (last_seg_lo) { *last_seg_lo = n_docs ? doc_offsets[n_docs - 1] : 0; *last_seg_hi = doc_offsets[n_docs]; }
        return encode_batch_locked(t, text, doc_offsets, n_docs, TD_MODE_ENCODE, out_tokens, out_capacity, out_offsets, n_tokens, unit, out_starts);
    }
    SpecialIndex ix;
    if ((rc = build_special_index(t, allowed_bytes, allowed_offsets, allowed_ids, n_allowed, ix))) return rc;
    // Batches of a MiB and more: the search runs on the device (td_special.hip; the same cuts, td_encode_device_with_special)
    // when the allowed set can be named by ids (no other special string shares an allowed one's id) and the caller does not
    // ask for the last segment (the single-string entry points do, for last_piece_token_len).
    if (t->opt.device_specials && !last_seg_lo && !out_starts && doc_offsets[n_docs] >= (1ll << 20) && t->H.pattern_kind != PATTERN_GENERIC && ix.count > 0) {
        std::vector<int32_t> ids;
        bool nameable = true;
        for (const auto& e : ix.ents) {
            ids.push_back(e.id);
            size_t carriers = 0;
            for (size_t k2 = 0; k2 < t->H.special_ids.size(); ++k2) carriers += t->H.special_ids[k2] == e.id && !t->H.special_strs[k2].empty();
            size_t listed = 0;
            for (const auto& e2 : ix.ents) listed += e2.id == e.id;
            if (carriers != listed) { nameable = false; break; }
            if (e.s->size() > 48) { nameable = false; break; }
        }
        if (nameable) {
            const int64_t n = doc_offsets[n_docs];
            if ((rc = ensure(t, t->h2d_text, (size_t)n + 64))) return rc;
            if ((rc = ensure(t, t->h2d_offs, (size_t)(n_docs + 1) * 8))) return rc;
            if ((rc = ensure(t, t->d_offsets, (size_t)(n_docs + 1) * 8))) return rc;
            const int64_t dev_cap = std::max<int64_t>(n, 1);
            if ((rc = ensure(t, t->d_tokens, (size_t)dev_cap * 4))) return rc;
            if ((rc = own_streams(t))) return rc;
            hipStream_t s = t->s_own;
            if ((rc = order_before(t, s))) return rc;
            if ((rc = special_search_prepare(t, ids.data(), (int64_t)ids.size(), n))) return rc;
            HIP_TRY(t, hipMemcpyAsync(t->h2d_text.p, text, (size_t)n, hipMemcpyHostToDevice, s));
            HIP_TRY(t, hipMemcpyAsync(t->h2d_offs.p, doc_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
            t->sp_active = t->sp_n != 0;
            rc = encode_device_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, TD_MODE_ENCODE, t->d_tokens.p, dev_cap, t->d_offsets.p, s);
            t->sp_active = false;
            if (rc) return rc;
            rc = device_status_locked(t, s, nullptr);
            if (rc == TD_E_SCRATCH) rc = TD_OK + 1000;  // (more candidates than the device list holds: the host search below)
            if (rc == TD_OK) {
                if ((rc = copy_wait(t, out_offsets, t->d_offsets.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
                const int64_t total = out_offsets[n_docs];
                t->enc_resident = true;
                if (t->enc_keep_resident) {  // (the caller reads d_tokens: td_encode_batch_span_label_rows)
                    if (n_tokens) *n_tokens = total;
                    return TD_OK;
                }
                return deliver_ids(t, total, out_capacity, out_tokens, n_tokens,
                                   [&] { return copy_wait(t, out_tokens, t->d_tokens.p, (size_t)total * 4, hipMemcpyDeviceToHost, s); });
            }
            if (rc != TD_OK + 1000) return rc;
        }
    }
    // 1. host: cut every document at the earliest occurrences of allowed special strings (tiktoken semantics; the
    //    reference's own loop, tiktoken.cpp:130-154,187-231, has iterator-invalidation UB).  Documents are independent:
    //    a few host threads take contiguous document ranges.
    std::vector<int64_t> starts, ends, doc_seg{0};
    std::vector<int32_t> seg_special;
    {
        const int64_t n = doc_offsets[n_docs];
        unsigned hw = std::thread::hardware_concurrency();
        int nth = (int)std::min<int64_t>(hw ? std::min(hw, 32u) : 4, std::max<int64_t>(1, n >> 22));  // one thread per 4 MiB, at most 32
        if (nth <= 1 || n_docs < 2 * nth || ix.count == 0) {
            for (int64_t d = 0; d < n_docs; ++d) {
                segment_document(ix, text, doc_offsets[d], doc_offsets[d + 1], starts, ends, seg_special);
                doc_seg.push_back((int64_t)seg_special.size());
            }
        } else {
            struct Part { std::vector<int64_t> starts, ends, per_doc; std::vector<int32_t> sp; };
            std::vector<Part> parts((size_t)nth);
            std::vector<std::thread> th;
            for (int k = 0; k < nth; ++k)
                th.emplace_back([&, k] {
                    Part& P = parts[(size_t)k];
                    const int64_t da = n_docs * k / nth, db = n_docs * (k + 1) / nth;
                    for (int64_t d = da; d < db; ++d) {
                        segment_document(ix, text, doc_offsets[d], doc_offsets[d + 1], P.starts, P.ends, P.sp);
                        P.per_doc.push_back((int64_t)P.sp.size());
                    }
                });
            for (auto& x : th) x.join();
            for (Part& P : parts) {
                const int64_t base = (int64_t)seg_special.size();
                starts.insert(starts.end(), P.starts.begin(), P.starts.end());
                ends.insert(ends.end(), P.ends.begin(), P.ends.end());
                seg_special.insert(seg_special.end(), P.sp.begin(), P.sp.end());
                for (int64_t v : P.per_doc) doc_seg.push_back(base + v);
            }
        }
    }
    const int64_t nseg = (int64_t)seg_special.size();
    if (last_seg_lo && nseg) { *last_seg_lo = starts[(size_t)nseg - 1]; *last_seg_hi = ends[(size_t)nseg - 1]; }
    // 2. device: all ordinary segments of all documents as ONE batch.  No special was cut out: the segments are the
    //    documents and the text goes down as it is; otherwise the segments are packed (the specials drop out).
    int64_t n_special = 0;
    for (int32_t v : seg_special) n_special += v >= 0;
    std::vector<int64_t> toffs((size_t)nseg + 1);
    int64_t ntok = 0;
    if (n_special == 0) {
        rc = encode_batch_locked(t, text, doc_offsets, n_docs, TD_MODE_ENCODE, out_tokens, out_capacity, out_offsets, &ntok, unit, out_starts);
        if (n_tokens) *n_tokens = ntok;
        return rc;
    }
    // The reference matches every segment with the text in front of it as left context (pcre2_match on text[0, end) from
    // start_offset, tiktoken.cpp:86-93): behind a special token \\A and ^ cannot match, \\b and a one-character look-behind see the
    // special's last character.  For a pattern with such assertions (rx_left_context) every segment that stands behind a
    // special token is sent down WITH that character in front of it, marked as context (gx_prefix): the matcher starts behind
    // it, sees it, and its bytes get no tokens.  (Round 3 refused the cut.)
    const bool ctx = t->H.rx_left_context && t->H.pattern_kind == PATTERN_GENERIC;
    std::vector<uint8_t> seg_text, prefix;
    std::vector<int64_t> seg_offs((size_t)nseg + 1, 0);
    {
        if (ctx) prefix.assign((size_t)nseg, 0);
        int64_t tot = 0;
        for (int64_t d = 0; d < n_docs; ++d)
            for (int64_t k = doc_seg[(size_t)d]; k < doc_seg[(size_t)d + 1]; ++k) {
                const int64_t lo = starts[(size_t)k], hi = ends[(size_t)k];
                if (ctx && k > doc_seg[(size_t)d] && hi > lo) {  // behind a special token of the same document
                    int64_t c = 1;
                    while (c < 4 && lo - c > doc_offsets[d] && (text[lo - c] & 0xC0u) == 0x80u) ++c;
                    prefix[(size_t)k] = (uint8_t)c;
                }
                tot += hi - lo + (ctx ? prefix[(size_t)k] : 0);
                seg_offs[(size_t)k + 1] = tot;
            }
        seg_text.resize((size_t)std::max<int64_t>(tot, 1));
        for (int64_t k = 0; k < nseg; ++k) {
            const int64_t pre = ctx ? prefix[(size_t)k] : 0, lo = starts[(size_t)k] - pre, hi = ends[(size_t)k];
            if (hi > lo) memcpy(seg_text.data() + seg_offs[(size_t)k], text + lo, (size_t)(hi - lo));
        }
    }
    std::vector<int32_t> toks((size_t)std::max<int64_t>(seg_offs[(size_t)nseg], 1));
    std::vector<int64_t> seg_starts(out_starts ? toks.size() : 0);  // (segment-relative, in bytes: shifted and converted below)
    if (ctx) t->gx_prefix_host = prefix.data();
    rc = encode_batch_locked(t, seg_text.data(), seg_offs.data(), nseg, TD_MODE_ENCODE, toks.data(), (int64_t)toks.size(), toffs.data(), &ntok,
                             TD_UNIT_BYTES, out_starts ? seg_starts.data() : nullptr);
    t->gx_prefix_host = nullptr;
    if (rc) return rc;
    // 3. stitch: offsets first (they do not need the capacity), then the ids
    const int64_t need = ntok + n_special;
    int64_t k = 0;
    for (int64_t d = 0; d < n_docs; ++d) {
        out_offsets[d] = k;
        for (int64_t sg = doc_seg[(size_t)d]; sg < doc_seg[(size_t)d + 1]; ++sg) k += toffs[(size_t)sg + 1] - toffs[(size_t)sg] + (seg_special[(size_t)sg] >= 0);
    }
    out_offsets[n_docs] = k;
    rc = deliver_ids(t, need, out_capacity, out_tokens, n_tokens, [&] {
        k = 0;
        for (int64_t sg = 0; sg < nseg; ++sg) {
            const int64_t cnt = toffs[(size_t)sg + 1] - toffs[(size_t)sg];
            if (cnt) memcpy(out_tokens + k, toks.data() + toffs[(size_t)sg], (size_t)cnt * 4);
            k += cnt;
            if (seg_special[(size_t)sg] >= 0) out_tokens[k++] = seg_special[(size_t)sg];
        }
        return (int)TD_OK;
    });
    if (rc) return rc;
    if (out_starts) {  // the same stitching for the starts: a segment's are shifted by where it stands in its document (its context in front of it)
        k = 0;
        for (int64_t d = 0; d < n_docs; ++d)
            for (int64_t sg = doc_seg[(size_t)d]; sg < doc_seg[(size_t)d + 1]; ++sg) {
                const int64_t shift = starts[(size_t)sg] - (ctx ? prefix[(size_t)sg] : 0) - doc_offsets[d];
                for (int64_t j = toffs[(size_t)sg]; j < toffs[(size_t)sg + 1]; ++j) out_starts[k++] = seg_starts[(size_t)j] + shift;
                if (seg_special[(size_t)sg] >= 0) out_starts[k++] = ends[(size_t)sg] - doc_offsets[d];
            }
        if (unit == TD_UNIT_CHARS) return chars_by_rank_locked(t, text, doc_offsets, n_docs, out_offsets, out_starts, need);
    }
    return TD_OK;
}

// Second element of the reference's return pair (tiktoken.cpp:185,213,218,225): number of ids of the last regex piece
// of the trailing ordinary segment text[s_lo, s_hi), 0 after a special.  Metadata only, derived on the host tables.
int32_t last_piece_token_len_host(td_tokenizer* t, const uint8_t* text, int64_t s_lo, int64_t s_hi) {
    if (s_hi <= s_lo) return 0;
    struct HostAcc {
        using pos_t = int64_t;
        const Tables* T; const uint8_t* p; int64_t lo, hi, lim;
        uint32_t byte(int64_t i) const { return i < hi ? p[i] : 0u; }
        bool doc(int64_t i) const { return i == lo; }
        uint32_t cf(int64_t i) const {
            if (i >= hi) return F_DOC;
            uint32_t v = classify_at(*T, *this, i);
            if (i == lo) v |= F_DOC;
            return v;
        }
    };
    const Tables hv = t->H.view();
    if (t->H.pattern_kind == PATTERN_GENERIC) {
        // the compiled pattern over the whole segment (no provable restart points): its last piece
        // (a segment behind a special token is matched with the special's last character in front of it, like the batch path)
        int64_t pre = 0;
        if (t->H.rx_left_context && s_lo > 0) {
            pre = 1;
            while (pre < 4 && s_lo - pre > 0 && (text[s_lo - pre] & 0xC0u) == 0x80u) ++pre;
        }
        struct SegAcc { const uint8_t* p; uint32_t byte(int64_t i) const { return p[i]; } } S{text + s_lo - pre};
        const RxProgram& P = *reinterpret_cast<const RxProgram*>(t->H.rx_program.data());
        const RxTables RT = rx_host_tables();
        const int64_t n = s_hi - s_lo + pre;
        int64_t ms = pre, me = pre;
        for (int64_t pos = pre; pos < n; pos = me) rx_next_piece(P, RT, S, pos, n, ms, me);
        const uint32_t len = (uint32_t)(me - ms);
        const uint8_t* pb = text + s_lo - pre + ms;
        std::vector<int32_t> tmp;
        const int32_t whole = (len == 1) ? t->H.byte_id[pb[0]] : piece_lookup(hv, piece_key_host(pb, len), len, [pb](uint32_t i) { return (uint32_t)pb[i]; });
        if (whole != NO_RANK) return 1;
        return merge_piece_host(hv, pb, len, tmp) == TD_OK ? (int32_t)tmp.size() : 0;
    }
    HostAcc A{&hv, text, s_lo, s_hi, s_hi + 4};
    // the last piece starts at or behind the last provable sync point of the segment: walk back to it instead of scanning
    // the whole segment (this runs on the host for every CoreBPE.encode call)
    int64_t p = s_lo;
    for (int64_t q = s_hi - 1; q > s_lo; --q)
        if (is_sync(A.cf(q - 1), A.cf(q), hv.pat_flags)) { p = q; break; }
    int64_t last = p;
    while (p < s_hi) { last = p; p = scan_piece(A, p, hv.pat_flags); }
    std::vector<int32_t> tmp;
    const uint32_t len = (uint32_t)(s_hi - last);
    const uint8_t* pb = text + last;
    const int32_t whole = (len == 1) ? t->H.byte_id[pb[0]]
                                     : piece_lookup(hv, piece_key_host(pb, len), len, [pb](uint32_t i) { return (uint32_t)pb[i]; });
    if (whole != NO_RANK) return 1;
    if (merge_piece_host(hv, pb, len, tmp) == TD_OK) return (int32_t)tmp.size();
    return 0;
}
}  // namespace

const int64_t no_offs[1] = {0};  // allowed_offsets of an empty allowed set

int td::encode_special_strs_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                   const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed, int32_t* out_tokens,
                                   int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens) {
    t->enc_resident = false;
    return encode_special_locked(t, text, doc_offsets, n_docs, allowed_bytes, n_allowed ? allowed_offsets : no_offs, nullptr, n_allowed,
                                 out_tokens, out_capacity, out_offsets, n_tokens, nullptr, nullptr);
}

extern "C" {

int td_encode_device_with_special(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                                  const int32_t* allowed_ids, int64_t n_allowed, void* d_out_tokens, int64_t out_capacity,
                                  void* d_out_offsets, void* hip_stream) {
    if (!t || n_allowed < 0 || (n_allowed > 0 && !allowed_ids)) return TD_E_INVALID;
    return locked(t, [&] {
        if (n_allowed == 0 || n_bytes == 0)
            return encode_device_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, TD_MODE_ENCODE, d_out_tokens, out_capacity, d_out_offsets,
                                        (hipStream_t)hip_stream);
        if (t->H.pattern_kind == PATTERN_GENERIC) {
            t->err = "td_encode_device_with_special: generic split patterns take their subjects from the document offsets; use td_encode_batch_with_special";
            return (int)TD_E_PATTERN;
        }
        int rc;
        if ((rc = special_search_prepare(t, allowed_ids, n_allowed, n_bytes))) return rc;
        t->sp_active = t->sp_n != 0;
        rc = encode_device_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, TD_MODE_ENCODE, d_out_tokens, out_capacity, d_out_offsets,
                                  (hipStream_t)hip_stream);
        t->sp_active = false;
        return rc;
    });
}

int td_encode_batch_with_special(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                 const int32_t* allowed_ids, int64_t n_allowed, int32_t* out_tokens, int64_t out_capacity,
                                 int64_t* out_offsets, int64_t* n_tokens) {
    if (!t || !doc_offsets || n_docs < 0 || n_allowed < 0 || (n_allowed > 0 && !allowed_ids) || !out_offsets || out_capacity < 0) return TD_E_INVALID;
    return locked(t, [&] {
        return encode_special_locked(t, text, doc_offsets, n_docs, nullptr, nullptr, allowed_ids, n_allowed, out_tokens, out_capacity,
                                     out_offsets, n_tokens, nullptr, nullptr);
    });
}

int td_encode_batch_with_special_strs(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                      const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                      int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens) {
    if (!t || !doc_offsets || n_docs < 0 || n_allowed < 0 || (n_allowed > 0 && (!allowed_bytes || !allowed_offsets)) || !out_offsets ||
        out_capacity < 0)
        return TD_E_INVALID;
    return locked(t, [&] {
        return encode_special_strs_locked(t, text, doc_offsets, n_docs, allowed_bytes, allowed_offsets, n_allowed, out_tokens, out_capacity,
                                          out_offsets, n_tokens);
    });
}

int td_encode_with_special(td_tokenizer* t, const uint8_t* text, int64_t n_bytes, const int32_t* allowed_ids,
                           int64_t n_allowed, int32_t* out_tokens, int64_t out_capacity, int64_t* n_tokens,
                           int32_t* last_piece_token_len) {
    if (!t || n_bytes < 0 || (n_bytes > 0 && !text) || n_allowed < 0 || (n_allowed > 0 && !allowed_ids) || out_capacity < 0) return TD_E_INVALID;
    return locked(t, [&] {
        const int64_t doc[2] = {0, n_bytes};
        int64_t offs[2] = {0, 0}, lo = 0, hi = 0;
        const int rc = encode_special_locked(t, text, doc, 1, nullptr, nullptr, allowed_ids, n_allowed, out_tokens, out_capacity, offs,
                                             n_tokens, &lo, &hi);
        if (rc == TD_OK && last_piece_token_len) *last_piece_token_len = last_piece_token_len_host(t, text, lo, hi);
        return rc;
    });
}

int td_encode_with_special_strs(td_tokenizer* t, const uint8_t* text, int64_t n_bytes, const uint8_t* allowed_bytes,
                                const int64_t* allowed_offsets, int64_t n_allowed, int32_t* out_tokens, int64_t out_capacity,
                                int64_t* n_tokens, int32_t* last_piece_token_len) {
    if (!t || n_bytes < 0 || (n_bytes > 0 && !text) || n_allowed < 0 || (n_allowed > 0 && (!allowed_bytes || !allowed_offsets)) || out_capacity < 0)
        return TD_E_INVALID;
    if (n_bytes == 0 && n_allowed == 0) {  // (no text, nothing allowed to validate: no ids, and no reason to wake the device)
        if (n_tokens) *n_tokens = 0;
        if (last_piece_token_len) *last_piece_token_len = 0;
        return TD_OK;
    }
    return locked(t, [&] {
        const int64_t doc[2] = {0, n_bytes};
        int64_t offs[2] = {0, 0}, lo = 0, hi = 0;
        const int rc = encode_special_locked(t, text, doc, 1, allowed_bytes, n_allowed ? allowed_offsets : no_offs, nullptr, n_allowed,
                                             out_tokens, out_capacity, offs, n_tokens, &lo, &hi);
        if (rc == TD_OK && last_piece_token_len) *last_piece_token_len = last_piece_token_len_host(t, text, lo, hi);
        return rc;
    });
}

int td_encode_batch_with_starts(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed, int unit,
                                int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* out_starts, int64_t* n_tokens) {
    if (!t || !doc_offsets || n_docs < 0 || n_allowed < 0 || (n_allowed > 0 && (!allowed_bytes || !allowed_offsets)) || !out_offsets ||
        out_capacity < 0 || (out_capacity > 0 && !out_starts) || (unit != TD_UNIT_BYTES && unit != TD_UNIT_CHARS) ||
        (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY) || (mode == TD_MODE_ORDINARY && n_allowed > 0))
        return TD_E_INVALID;
    if (unit == TD_UNIT_CHARS && doc_offsets[n_docs] >= (1ll << 32))
        return fail_unlocked(t, TD_E_INVALID, "td_encode_batch_with_starts: character starts need less than 4 GiB of text a call");
    return locked(t, [&] {
        if (n_allowed == 0)
            return encode_batch_locked(t, text, doc_offsets, n_docs, mode, out_tokens, out_capacity, out_offsets, n_tokens, unit, out_starts);
        return encode_special_locked(t, text, doc_offsets, n_docs, allowed_bytes, allowed_offsets, nullptr, n_allowed, out_tokens,
                                     out_capacity, out_offsets, n_tokens, nullptr, nullptr, unit, out_starts);
    });
}

}  // extern "C"
