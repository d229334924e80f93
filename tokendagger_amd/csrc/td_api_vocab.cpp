// Vocabulary files behind the C ABI: td_vocab wraps td::VocabData (td_vocab.cpp); td_create_from_vocab hands its arrays to td_create.
#include "../../include/tokendagger_hip.h"
#include "td_vocab.h"

using namespace td;

struct td_vocab {
    td::VocabData d;
};

extern "C" {

int td_vocab_create(td_vocab** out) {
    if (!out) return TD_E_INVALID;
    *out = new td_vocab;
    return TD_OK;
}
void td_vocab_destroy(td_vocab* v) { delete v; }
const char* td_vocab_error(const td_vocab* v) { return v ? v->d.err.c_str() : "null td_vocab"; }

int td_vocab_load_tiktoken(td_vocab* v, const char* path) {
    if (!v || !path) return TD_E_INVALID;
    return load_tiktoken_model(path, v->d) ? TD_OK : TD_E_VOCAB;
}
int td_vocab_load_hf_special(td_vocab* v, const char* path, int also_mergeable) {
    if (!v || !path) return TD_E_INVALID;
    return load_hf_added_tokens(path, v->d, also_mergeable != 0) ? TD_OK : TD_E_VOCAB;
}
int td_vocab_load_tekken(td_vocab* v, const char* path) {
    if (!v || !path) return TD_E_INVALID;
    return load_tekken_json(path, v->d) ? TD_OK : TD_E_VOCAB;
}
int td_vocab_load_json(td_vocab* v, const char* vocab_json_path, const char* special_json_path) {
    if (!v || (!vocab_json_path && !special_json_path)) return TD_E_INVALID;
    return load_wrapper_json(vocab_json_path ? vocab_json_path : "", special_json_path ? special_json_path : "", v->d) ? TD_OK
                                                                                                                      : TD_E_VOCAB;
}
int td_vocab_set_pattern(td_vocab* v, const char* pat_str) {
    if (!v || !pat_str) return TD_E_INVALID;
    v->d.pattern = pat_str;
    return TD_OK;
}
const char* td_vocab_pattern(const td_vocab* v) { return v ? v->d.pattern.c_str() : ""; }

int td_vocab_arrays(const td_vocab* v, int which, const uint8_t** bytes, const int64_t** offsets, const int32_t** ranks,
                    int64_t* n) {
    if (!v || (which != 0 && which != 1)) return TD_E_INVALID;
    const td::TokenList& l = which ? v->d.special : v->d.regular;
    static const uint8_t none = 0;
    if (bytes) *bytes = l.bytes.empty() ? &none : l.bytes.data();
    if (offsets) *offsets = l.offsets.data();
    if (ranks) *ranks = l.ranks.data();
    if (n) *n = l.size();
    return TD_OK;
}

int td_create_from_vocab(const td_vocab* v, int device, td_tokenizer** out) {
    if (!v || !out) return TD_E_INVALID;
    const uint8_t *b = nullptr, *sb = nullptr;
    const int64_t *o = nullptr, *so = nullptr;
    const int32_t *r = nullptr, *sr = nullptr;
    int64_t n = 0, ns = 0;
    td_vocab_arrays(v, 0, &b, &o, &r, &n);
    td_vocab_arrays(v, 1, &sb, &so, &sr, &ns);
    return td_create(v->d.pattern.c_str(), n, b, o, r, ns, sb, so, sr, device, out);
}

}  // extern "C"
