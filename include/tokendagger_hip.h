/*
 * tokendagger_hip.h — C ABI of the MI355X-native tokenizer hot path (libtokendagger_hip.so).
 *
 * This is the drop-in boundary for the ONE path this repository accelerates: raw UTF-8 text ->
 * regex pre-tokenization -> byte-pair merge -> token ids (reference: tiktoken::CoreBPE,
 * /root/reference/src/tiktoken/tiktoken.hpp:38-88).  Plain pointers and sizes only; no torch,
 * pybind or C++ types cross it.  Every entry point names the reference interface it replaces.
 * INTEGRATION.md shows the reference-side binding (pybind11 / ctypes) a maintainer would add.
 *
 * Conventions
 *   - every function returns TD_OK (0) or a TD_E_* code; td_last_error() gives the message
 *     (the C ABI equivalent of the reference's `TiktokenError` exception, tiktoken.hpp:32-35);
 *   - text is UTF-8, documents are concatenated: document d = text[doc_offsets[d], doc_offsets[d+1]),
 *     doc_offsets[0] == 0, doc_offsets[n_docs] == total bytes, offsets are int64;
 *   - token ids are int32 and equal the `rank` values given at construction;
 *   - there is no CPU fallback: without a usable HIP device td_create fails.
 */
#ifndef TOKENDAGGER_HIP_H
#define TOKENDAGGER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_OK 0
#define TD_E_INVALID 1      /* bad argument */
#define TD_E_PATTERN 2      /* pat_str uses regex syntax outside what the device pre-tokenizer implements (td_last_error says which) */
#define TD_E_VOCAB 3        /* vocabulary cannot be represented */
#define TD_E_UNKNOWN_BYTE 4 /* input contains a byte / part that is not in the vocabulary
                               (reference: TiktokenError "No value found for pair", tiktoken.cpp:364) */
#define TD_E_CAPACITY 5     /* output buffer too small */
#define TD_E_SCRATCH 6      /* long-piece scratch exhausted; raise it with td_set_option */
#define TD_E_HIP 7          /* HIP runtime failure */
#define TD_E_BAD_TOKEN 8    /* decode: id not in the vocabulary (reference: "Invalid token for decoding", tiktoken.cpp:249) */
#define TD_E_SPECIAL 9      /* allowed special token not in the special vocabulary (tiktoken.cpp:178-180) */

/* encode modes */
#define TD_MODE_ENCODE 0    /* CoreBPE::encode(text, {}): whole-piece lookup, then merge  (tiktoken.cpp:169-234) */
#define TD_MODE_ORDINARY 1  /* CoreBPE::encode_ordinary(text): merge only               (tiktoken.cpp:156-167) */

typedef struct td_tokenizer td_tokenizer;

/*
 * Replaces CoreBPE::CoreBPE(pattern, vocab, special_vocab)  (tiktoken.hpp:48-67, py_binding.cpp:22-24).
 * The vocabulary is passed as concatenated token bytes + n+1 offsets + n ranks (what a list of
 * VocabItem{rank, token_bytes} holds, tiktoken.hpp:12-16); specials likewise (token_string, rank).
 * Builds the device tables and uploads them to HIP device `device` (-1: current device).
 * pat_str (init_regex, tiktoken.cpp:47-68): the known tokenizer patterns (o200k / Llama-4, tekken, cl100k_base / Llama-3, Qwen2, GPT-2)
 * have kernels of their own; any other pattern within the backtracking subset listed in tokendagger_amd/csrc/td_regex.h is
 * compiled and matched with PCRE2's semantics (text it skips gets no tokens, tiktoken.cpp:86-122), in parallel inside a
 * document too (speculative chunks of 64 B .. 1 KiB, checked against their predecessors);
 * anything else is TD_E_PATTERN.  There is no CPU regex fallback.
 */
int td_create(const char* pat_str, int64_t n_vocab, const uint8_t* token_bytes, const int64_t* token_offsets,
              const int32_t* ranks, int64_t n_special, const uint8_t* special_bytes,
              const int64_t* special_offsets, const int32_t* special_ids, int device, td_tokenizer** out);

/* A second handle on the SAME tables: its own lock, workspace, control block and streams, but the device tables td_create
 * uploaded (and their host copies) are shared, not copied — what a host thread per HIP stream needs to run encodes
 * concurrently (the reference shares one CoreBPE between the threads of its pool, tokendagger/wrapper.py:212-235, each with
 * its own match data, tiktoken.cpp:13-45).  Options set on `src` so far are inherited.  The tables are freed with the last
 * handle that shares them; every handle is destroyed with td_destroy, in any order. */
int td_clone(td_tokenizer* src, td_tokenizer** out);

/* Replaces CoreBPE::~CoreBPE (tiktoken.hpp:69-73). */
void td_destroy(td_tokenizer* t);

/* Message of the calling thread's last failing call on this handle ("" if none; t == NULL: last td_create failure of
 * this thread).  The pointer stays valid until the same thread's next failing call.
 *
 * Threads and streams: a handle may be shared by host threads; calls serialise on one internal lock.  All calls of a
 * handle share ONE device workspace: work of a handle is ordered across streams by the library (a call on another
 * stream than the previous call's waits, on the device, for that call's kernels), so asynchronous calls on different
 * streams do not overlap each other — use one handle per stream for concurrency (td_clone: without a second copy of the tables).  Every entry point leaves the
 * caller's current HIP device as it found it.
 *
 * The legacy (null) stream: the library never uses it on its own — copies it waits for, table uploads and the host-buffer
 * entry points run on a private non-blocking stream of the handle, results come back through pinned memory — so it neither
 * synchronises with the application's blocking streams nor breaks a stream capture another thread has open.  Kernels are
 * launched on the null stream only where the CALLER passes hip_stream == NULL to a *_device entry point.  (Workspace growth
 * calls hipMalloc / hipFree: td_reserve up front if the application captures in global mode.) */
const char* td_last_error(const td_tokenizer* t);

/*
 * Bulk encode from HOST buffers: the batched form of CoreBPE::encode / encode_ordinary over n_docs
 * independent documents (the reference reaches the same through a thread pool over single calls,
 * tokendagger/wrapper.py:212-235).  out_tokens (capacity out_capacity ids) receives all ids,
 * out_offsets[n_docs+1] the per-document token offsets, *n_tokens the total.  If the capacity is
 * too small the call fails with TD_E_CAPACITY and *n_tokens holds the required size.
 * Synchronous.  Three paths by size: inputs of at most 4 KiB (and 1024 documents) take ONE kernel launch that reads and writes pinned
 * host memory directly (TD_OPT_SMALL_PATH); up to 4 MiB (and 262 144 documents) text and offsets travel through one pinned buffer and one
 * asynchronous copy, the step's last kernels write ids and offsets straight into pinned host memory, and the host waits on a sequence
 * number instead of stream synchronisations (TD_MID_PATH=0 in the environment at td_create time: the copy-and-synchronise path that
 * inputs between 4 and 32 MiB still take); from half of TD_OPT_PIPE_CHUNK_BYTES on (default: 32 MiB) a four-slot pipeline of pinned bounce
 * buffers (host copy || H2D || kernels || ids out by a kernel || host copy, TD_OPT_PIPE_*: about 4 x (64 + 256) MiB of device memory
 * plus the pinned buffers while such calls are made).
 */
int td_encode_batch(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                    int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens);

/*
 * The same on DEVICE-resident buffers, asynchronously on `hip_stream` (a hipStream_t; NULL = the
 * default stream): d_text[n_bytes] (uint8), d_doc_offsets[n_docs+1] (int64), d_out_tokens[out_capacity]
 * (int32), d_out_offsets[n_docs+1] (int64; element n_docs = total token count).  Nothing is
 * synchronised; call td_device_status() after the stream has drained to learn about device-side
 * errors.  Workspace is (re)allocated on demand — call td_reserve() first to keep hipMalloc out of
 * a timed or captured region.
 */
int td_encode_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets,
                     int64_t n_docs, int mode, void* d_out_tokens, int64_t out_capacity, void* d_out_offsets,
                     void* hip_stream);

/* Pre-allocates workspace for inputs up to max_bytes / max_docs. */
int td_reserve(td_tokenizer* t, int64_t max_bytes, int64_t max_docs);

/* Synchronises `hip_stream` and returns the device error raised by calls made since the last status
 * check (TD_OK if none); *err_pos (optional) receives the byte offset it refers to. */
int td_device_status(td_tokenizer* t, void* hip_stream, int64_t* err_pos);

/*
 * Replaces CoreBPE::decode_bytes(tokens) (tiktoken.cpp:236-255, py_binding.cpp:40-44) for host
 * buffers: ids -> concatenated bytes.  *n_bytes receives the size (also on TD_E_CAPACITY).
 */
int td_decode_bytes(td_tokenizer* t, const int32_t* tokens, int64_t n_tokens, uint8_t* out, int64_t out_capacity,
                    int64_t* n_bytes);

/*
 * Replaces CoreBPE::encode(text, allowed_special) with a NON-empty allowed set (tiktoken.cpp:169-234,
 * find_next_special_token :130-154) with tiktoken semantics: the text is cut at the earliest
 * occurrences of allowed special strings, ordinary segments go through the kernels, each special
 * contributes its id.  allowed_ids lists the special ids that are allowed.
 * *last_piece_token_len (optional) is the second element of the reference's return pair.
 */
int td_encode_with_special(td_tokenizer* t, const uint8_t* text, int64_t n_bytes, const int32_t* allowed_ids,
                           int64_t n_allowed, int32_t* out_tokens, int64_t out_capacity, int64_t* n_tokens,
                           int32_t* last_piece_token_len);

/* The same over a batch of documents: every document is cut at its allowed special tokens (one pass, all literals at
 * once), all ordinary segments of all documents go to the GPU as ONE batch, ids and per-document offsets come back
 * stitched.  *n_tokens = ids needed (also on TD_E_CAPACITY). */
int td_encode_batch_with_special(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                 const int32_t* allowed_ids, int64_t n_allowed, int32_t* out_tokens, int64_t out_capacity,
                                 int64_t* out_offsets, int64_t* n_tokens);

/* The same two calls with the allowed set given as the special-token STRINGS themselves (concatenated UTF-8 bytes +
 * n_allowed+1 offsets), which is how tiktoken's `allowed_special` names them: exactly the listed literals are cut
 * out.  (With ids, every special string that carries a listed id is allowed — two strings may share one id.)
 * A string that is not a special token fails with TD_E_SPECIAL, like tiktoken.cpp:178-180. */
int td_encode_with_special_strs(td_tokenizer* t, const uint8_t* text, int64_t n_bytes, const uint8_t* allowed_bytes,
                                const int64_t* allowed_offsets, int64_t n_allowed, int32_t* out_tokens, int64_t out_capacity,
                                int64_t* n_tokens, int32_t* last_piece_token_len);
int td_encode_batch_with_special_strs(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                      const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                      int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens);

/* Introspection (tests, benchmarks). */
#define TD_INFO_N_PAIRS 1        /* entries of the (id,id)->rank pair table */
#define TD_INFO_MERGE_CLOSED 2   /* 1 if encode == encode_ordinary for every input with this vocab */
#define TD_INFO_MAX_ID 3
#define TD_INFO_TILE_BYTES 4
#define TD_INFO_WORKSPACE_BYTES 5
#define TD_INFO_N_SPECIAL 6
#define TD_INFO_LONG_PIECES 7    /* long pieces seen by the last td_encode_batch call */
#define TD_INFO_FAR_PIECES 8     /* pieces whose end the pre-tokenizer's window could not see (td_split_far_pieces), last call */
#define TD_INFO_DEFERRED_TILES 9 /* token tiles (4 KiB) the fused tile loop left to td_probe_tiles, last call (as of the last td_device_status) */
#define TD_INFO_FLAGGED_TILES 10 /* token tiles whose missed pieces went to td_merge_pieces, last call */
#define TD_INFO_LB_TIMEOUTS 12   /* ... and tiles it staged because their output base was not known in time (bounded look-back), last call */
#define TD_INFO_REPEATS 13       /* missed pieces whose ids were taken from another piece with the same bytes (TD_OPT_DEDUPE), last call */
#define TD_INFO_LISTED_PIECES 14 /* ... and missed pieces of the same tiles that were merged themselves, last call */
#define TD_INFO_CHAR_SEEDS 15    /* characters of 2..3 bytes this vocabulary allows to enter the merge of a long piece as one part (td_common.h) */
#define TD_INFO_SPARSE 16        /* 1: the last td_encode_device call of the handle took the sparse launch sequence (TD_OPT_SPARSE), 0: the dense one */
#define TD_INFO_WS_FILLED_BYTES 17 /* bytes this handle has filled since it was made (TD_OPT_WS_FILL): at allocation and in front of steps */
#define TD_INFO_SMALL_ENCODES 18          /* host calls of at most 4 KiB and 1024 documents the one-launch kernel (td_small_encode / td_small_resident) answered itself, an error it reported included, since the handle was made (a td_clone handle starts at 0) */
#define TD_INFO_SMALL_ENCODE_HANDBACKS 19 /* ... and calls it handed back to the general path (a piece above 1024 bytes, a full list) */
#define TD_INFO_SMALL_DECODES 20          /* td_decode_bytes calls of at most 1024 ids td_small_decode answered itself, since the handle was made */
#define TD_INFO_SMALL_DECODE_HANDBACKS 21 /* ... and calls it handed back (more than 16 384 bytes) */
#define TD_INFO_DIRECT_TILES 11 /* pre-tokenizer tiles (8 KiB) whose ids the fused tile loop wrote straight to the output (TD_OPT_DIRECT), last call */
int64_t td_info(const td_tokenizer* t, int what);

/*
 * CoreBPE::encode(text, allowed_special) (tiktoken.cpp:169-234) on DEVICE-RESIDENT text, asynchronous like td_encode_device: the
 * allowed special tokens (by id) are searched for and cut out on the device — scanning forward, the longest allowed literal
 * that starts at a position is replaced by its id, the text between two cuts is tokenized as a subject of its own
 * (td_special.hip; the same results as td_encode_batch_with_special, whose search runs on host threads).  One allowed set is
 * kept on the device per handle; a call with a different set first waits for the previous call's kernels.  Patterns of the
 * scanner family only (generic patterns: TD_E_PATTERN).  Limit of the device search: an allowed literal of more than 48 bytes
 * fails with TD_E_INVALID and a message that says so (TD_E_SPECIAL stays "no such special token"); the host-buffer entry
 * points (td_encode_batch_with_special*) have no such limit — they search on host threads then.
 */
int td_encode_device_with_special(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                                  const int32_t* allowed_ids, int64_t n_allowed, void* d_out_tokens, int64_t out_capacity,
                                  void* d_out_offsets, void* hip_stream);

/* ---- per-token start offsets (td_offsets.hip) ----------------------------------------------------------------------------
 * The START of a token is where its text begins in its own document:
 *   TD_UNIT_BYTES  the offset of its first byte in the document's UTF-8 bytes;
 *   TD_UNIT_CHARS  tiktoken's decode_with_offsets rule in code points: with chars(b) = the bytes of doc[0, b) that are not
 *                  continuation bytes (0x80..0xBF), start = max(0, chars(b) - (doc[b] is a continuation byte)) — a token that
 *                  begins inside a character points at that character; for text that is valid UTF-8 the index into the
 *                  decoded string.
 * The end of a token in bytes is start + its byte length (td_token_bytes).  Starts are computed on the device: a segmented
 * scan of per-id byte lengths or character counts (a per-id table built at td_create, special tokens included); a generic
 * pattern that skips text maps the documents where it did through a bitmap of the bytes it covered.  Errors are reported
 * like the other entry points': an id outside the vocabulary is TD_E_BAD_TOKEN with its index, a too small output
 * TD_E_CAPACITY. */
#define TD_UNIT_BYTES 0
#define TD_UNIT_CHARS 1

/* Starts from ids alone, by the covered rule (every document's bytes are its tokens' bytes concatenated): the offsets of
 * decode_with_offsets, and the encode offsets of any pattern that skips no text.  tokens[n_tokens] holds the ids of all
 * documents concatenated, tok_offsets[n_docs+1] the first id of every document; out_starts has room for n_tokens starts
 * (tok_offsets[n_docs] > n_tokens: TD_E_CAPACITY).  Synchronous. */
int td_token_starts(td_tokenizer* t, const int32_t* tokens, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, int unit,
                    int64_t* out_starts);
/* The same on device buffers, asynchronously on hip_stream; errors surface through td_device_status. */
int td_token_starts_device(td_tokenizer* t, const void* d_tokens, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs, int unit,
                           void* d_out_starts, void* hip_stream);

/* td_encode_batch_with_special_strs (mode TD_MODE_ENCODE) / td_encode_batch (n_allowed == 0) that also returns the start of
 * every id: out_starts (int64, room for out_capacity) in `unit`.  The ids equal those of the entry points it stands for.
 * Every pattern kind: the family's, generic patterns (also where they skip text) and allowed special tokens (a special's
 * start is where its literal stands; the starts of the text between two specials are shifted by where it stands).
 * TD_MODE_ORDINARY takes no allowed set (TD_E_INVALID).  Synchronous; it takes the copy-and-synchronise path at every size
 * (not the one-launch, mid-size or pipelined forms of td_encode_batch).  TD_UNIT_CHARS: less than 4 GiB of text a call. */
int td_encode_batch_with_starts(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed, int unit,
                                int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* out_starts, int64_t* n_tokens);

/* td_encode_device that also writes d_out_starts (int64, room for out_capacity): device-resident and asynchronous like
 * td_encode_device, every pattern kind, no special tokens.  The starts are launched behind the encode on the same stream
 * (a generic pattern's skipped text is read from the workspace of this very call).  TD_UNIT_CHARS: n_bytes below 4 GiB. */
int td_encode_device_with_starts(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int mode,
                                 int unit, void* d_out_tokens, int64_t out_capacity, void* d_out_offsets, void* d_out_starts,
                                 void* hip_stream);

/* ---- training rows (td_rows.hip) -----------------------------------------------------------------------------------------
 * Encoded documents -> rows of a fixed length S.  Input: ids[n_tokens] (int32) and tok_offsets[n_docs+1] (int64), what
 * td_encode_batch / td_encode_device produce; L_d = tok_offsets[d+1] - tok_offsets[d].  b = (bos_id >= 0), e = (eos_id >= 0).
 *
 * TD_ROWS_CONCAT  every document becomes [BOS] ids... [EOS], n_d = b + L_d + e slots (an empty document without BOS and EOS: 0
 *   slots), concatenated in document order into a stream of T = tok_offsets[n_docs] + n_docs * (b + e) slots; document d starts
 *   at base_d = tok_offsets[d] + d * (b + e).  The stream is cut into rows of S: rows = ceil(T / S), the tail padded with pad_id;
 *   with TD_ROWS_DROP_LAST rows = floor(T / S) and the partial row is dropped.  R = min(T, rows * S) slots are real.
 *     positions[rows * S]  a slot's index inside its SEGMENT; segments are the pieces of [0, R) cut at every document start and
 *                          every row start; pad slots are 0.
 *     aux = cu_seqlens     the sorted segment boundaries 0 ... R without duplicates (n_seg + 1 entries, never a zero-length
 *                          segment): the cu_seqlens of variable-length attention over the flattened [rows * S] batch.
 * TD_ROWS_PAD  one row per document (rows = n_docs): [BOS] body [EOS] then pad_id, the body truncated to min(L_d, S - b - e)
 *   ids (S < b + e: TD_E_INVALID), so a truncated document still ends with EOS (Hugging Face's truncation with special tokens).
 *     positions            0 .. len - 1, pad slots 0.
 *     aux = lengths        [n_docs] the real slots of every row (int32).
 *   Not allowed with TD_ROWS_DROP_LAST.
 * counts[4] (int64) = {rows, R (real slots), n_seg (PAD: rows with at least one slot), documents truncated (PAD)}.
 * bos_id / eos_id: -1 for none, otherwise an id of the vocabulary, ordinary or special (else TD_E_BAD_TOKEN); pad_id: any int32.
 * seq_len: 1 .. 2^31 - 1.  With cu_seqlens requested, rows_capacity * seq_len must stay below 2^31 (its entries are int32). */
#define TD_ROWS_CONCAT 0
#define TD_ROWS_PAD 1
#define TD_ROWS_DROP_LAST 1 /* flags */
typedef struct td_rows_spec {
    int64_t layout;  /* TD_ROWS_CONCAT / TD_ROWS_PAD */
    int64_t seq_len; /* S */
    int64_t bos_id;  /* -1: none */
    int64_t eos_id;  /* -1: none */
    int64_t pad_id;
    int64_t flags;   /* TD_ROWS_DROP_LAST (CONCAT only) */
} td_rows_spec;

/* Rows from DEVICE buffers, asynchronously on hip_stream.  d_out_ids has room for rows_capacity rows of S; d_positions (same
 * size) and d_aux (CONCAT: cu_seqlens, room for n_docs + rows_capacity + 1 entries; PAD: lengths, n_docs entries) may be NULL;
 * d_counts (4 int64) is required.  The host does not know T, so the kernels check the capacity: more rows than rows_capacity
 * raise TD_E_CAPACITY with err_pos (td_device_status) = the rows needed and counts[0] = the same, and nothing is written into
 * the outputs.  tok_offsets[n_docs] > n_tokens is TD_E_INVALID on the device too; tok_offsets must start at 0 and not decrease
 * (the host form checks that; here no id outside [0, n_tokens) is read whatever they hold). */
int td_make_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                        const td_rows_spec* spec, void* d_out_ids, int64_t rows_capacity, void* d_positions, void* d_aux,
                        void* d_counts, void* hip_stream);
/* The same on host buffers, synchronously.  tok_offsets is checked like every host entry point's offsets.  The rows are known
 * on the host: a capacity below them fails before any launch with TD_E_CAPACITY and counts[0] = the rows needed. */
int td_make_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                 const td_rows_spec* spec, int32_t* out_ids, int64_t rows_capacity, int32_t* out_positions, int32_t* out_aux,
                 int64_t* counts);
/* td_encode_batch (mode TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and td_make_rows in one call: the ids stay
 * in the handle's workspace between the two.  Synchronous; it takes the copy-and-synchronise path at every size (not the
 * one-launch, mid-size or pipelined forms of td_encode_batch).  Callers that need allowed specials encode first
 * (td_encode_batch_with_special_strs) and call td_make_rows. */
int td_encode_batch_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                         const td_rows_spec* spec, int32_t* out_ids, int64_t rows_capacity, int32_t* out_positions, int32_t* out_aux,
                         int64_t* counts);

/* ---- whole documents packed into rows by best-fit decreasing (td_pack.hip) ------------------------------------------------
 * td_rows_spec with layout = TD_ROWS_BESTFIT; flags 0 or TD_ROWS_TRUNCATE (TD_ROWS_DROP_LAST is invalid here).  bos / eos / pad
 * are checked as for the other layouts.  The td_make_rows* entry points reject this layout and this flag.
 *   Slots: document d has n_d = b + L_d + e slots, [BOS] ids [EOS] (an empty document without BOS and EOS: none, no segment).
 *     TD_ROWS_TRUNCATE: the body is cut to min(L_d, S - b - e) ids, so the document still ends with EOS (S < b + e: TD_E_INVALID).
 *     Otherwise (split) a document with n_d > S is cut at multiples of S of its own slots: floor(n_d / S) full chunks and a
 *     remainder chunk of n_d mod S slots (if > 0).
 *   Items are all chunks, sorted by length descending, then document ascending, then chunk ascending.  In that order each goes
 *   into the row whose free slot count is the smallest one >= its length (ties: the lowest row index); if no row has room, a
 *   new row is appended.  Rows are numbered in the order they were opened, so the full chunks are rows 0 .. F - 1 in (document,
 *   chunk) order.  Inside a row the segments sit in placement order from slot 0 and pad_id fills the tail.
 *   Outputs (td_pack_outputs; every field but ids may be NULL):
 *     ids          int32 [rows * S]
 *     positions    int32 [rows * S]  the index inside the segment (a split document's later chunks restart at 0); pad slots 0
 *     cu_seqlens   int32 the segment boundaries over the flattened [rows * S]: every real segment and every row's pad tail is a
 *                  segment; the last entry is rows * S.  Room: n_docs + 2 * rows_capacity + 1 entries, and rows_capacity * S < 2^31.
 *     row_lengths  int32 [rows]  the real slots of every row
 *     seg_docs     int64, one per cu_seqlens segment: the document, or -1 for a pad tail.  Room: n_docs + 2 * rows_capacity.
 *   counts[4] (int64) = {rows, R (real slots), segments (pad tails included), documents cut (split or truncated)}.
 *   Too few rows: TD_E_CAPACITY with counts[0] = the rows needed, and nothing is written to any output.  A caller who cannot
 *   plan first may use rows <= floor(2 * T / S) + 1 with T = n_ids + n_docs * (b + e): best-fit decreasing never leaves two
 *   rows at most half full.  n_docs < 2^31. */
#define TD_ROWS_BESTFIT 2
#define TD_ROWS_TRUNCATE 2 /* flags (TD_ROWS_BESTFIT only) */
typedef struct td_pack_outputs {
    int32_t* ids;
    int32_t* positions;
    int32_t* cu_seqlens;
    int32_t* row_lengths;
    int64_t* seg_docs;
} td_pack_outputs;

/* The counts of the packing, on the host, from tok_offsets[n_docs + 1] alone (no handle, no device).  doc_row / doc_slot (each
 * [n_docs], may be NULL): the row and in-row slot of the document's packed chunk (its only chunk, or its remainder when split);
 * -1 where it has none.  tok_offsets must start at 0 and not decrease. */
int td_pack_plan(const int64_t* tok_offsets, int64_t n_docs, const td_rows_spec* spec, int64_t* counts, int64_t* doc_row,
                 int64_t* doc_slot);
/* Host buffers, synchronously.  tok_offsets is checked like every host entry point's offsets. */
int td_pack_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                 const td_rows_spec* spec, const td_pack_outputs* host_out, int64_t rows_capacity, int64_t* counts);
/* Device buffers.  Unlike every other rows entry point this one SYNCHRONISES ONCE: it reads a small table of run lengths back to
 * plan the rows, so it waits for the caller's earlier work on hip_stream.  counts (HOST memory), capacity errors and offset
 * errors (tok_offsets decreasing or negative, tok_offsets[n_docs] > n_tokens) come back synchronously, before anything is
 * written; the kernels that write dev_out are then enqueued on hip_stream and run asynchronously. */
int td_pack_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                        const td_rows_spec* spec, const td_pack_outputs* dev_out, int64_t rows_capacity, int64_t* counts,
                        void* hip_stream);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and td_pack_rows in one call: the ids stay on
 * the device.  Synchronous. */
int td_encode_batch_pack_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                              const td_rows_spec* spec, const td_pack_outputs* host_out, int64_t rows_capacity, int64_t* counts);

/* ---- overlapping window rows for documents longer than seq_len (td_windows.hip) -------------------------------------------
 * One document per row, and every id kept: a document that does not fit continues in further rows of its own, and consecutive
 * rows of a document repeat `overlap` ids (Hugging Face: stride + return_overflowing_tokens + overflow_to_sample_mapping).
 * td_rows_spec with layout = TD_ROWS_WINDOWS and flags = 0 (TD_ROWS_DROP_LAST and TD_ROWS_TRUNCATE are TD_E_INVALID here);
 * bos / eos / pad are checked as for the other layouts; `overlap` is an argument of its own.  The td_make_rows* and td_pack_*
 * entry points reject this layout.
 *   b = (bos_id >= 0), e = (eos_id >= 0), body room C = S - b - e, step = C - overlap.  C < 1, overlap < 0 or overlap >= C:
 *   TD_E_INVALID.
 *   Document d has w_d = max(1, ceil((L_d - overlap) / step)) windows: L_d <= C gives one, and an empty document has a row too.
 *   Window k holds the document's ids [k * step, min(L_d, k * step + C)), so every window after the first repeats exactly
 *   `overlap` ids and brings at least one new id, and the union of a document's windows is the document.
 *   Window k of document d is row first_row[d] + k, first_row the exclusive prefix sum of w; rows = first_row[n_docs].
 *   A row is [BOS] body [EOS] then pad_id; every window has its own BOS and EOS.
 *   Outputs (td_window_outputs; every field but ids may be NULL):
 *     ids          int32 [rows * S]
 *     positions    int32 [rows * S]  0 .. len - 1 inside the row, pad slots 0
 *     row_lengths  int32 [rows]      the real slots of the row
 *     row_docs     int64 [rows]      the row's document
 *     row_starts   int64 [rows]      k * step: the index of the row's first body id inside its document.  With the starts of
 *                                    td_token_starts* the row's text begins at starts[tok_offsets[row_docs[r]] + row_starts[r]].
 *   counts[4] (int64) = {rows, R (real slots), documents with more than one window, the largest w_d}.
 *   With overlap = 0 and no L_d > C, ids, positions and row_lengths are TD_ROWS_PAD's byte for byte.
 *   n_docs < 2^31, seq_len 1 .. 2^31 - 1; rows * S may exceed 2^31. */
#define TD_ROWS_WINDOWS 3
typedef struct td_window_outputs {
    int32_t* ids;
    int32_t* positions;
    int32_t* row_lengths;
    int64_t* row_docs;
    int64_t* row_starts;
} td_window_outputs;

/* The counts, on the host, from tok_offsets[n_docs + 1] alone (no handle, no device); first_row[n_docs + 1] may be NULL.
 * tok_offsets must start at 0 and not decrease. */
int td_window_plan(const int64_t* tok_offsets, int64_t n_docs, const td_rows_spec* spec, int64_t overlap, int64_t* counts,
                   int64_t* first_row);
/* Host buffers, synchronously.  tok_offsets is checked like every host entry point's offsets.  The rows are known on the host:
 * a capacity below them fails before any launch with TD_E_CAPACITY and counts[0] = the rows needed. */
int td_window_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                   const td_rows_spec* spec, int64_t overlap, const td_window_outputs* host_out, int64_t rows_capacity, int64_t* counts);
/* DEVICE buffers, asynchronously on hip_stream: no synchronisation and no read-back.  d_counts (4 int64) is device memory.  More
 * rows than rows_capacity raise TD_E_CAPACITY through td_device_status with err_pos = the rows needed and counts[0] = the same,
 * and nothing is written to any output.  tok_offsets that decrease, are negative or end above n_tokens raise TD_E_INVALID
 * (err_pos: a document with such offsets) and nothing is written either; whatever they hold, no id outside [0, n_tokens) is
 * read and nothing is written outside the capacities given. */
int td_window_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                          const td_rows_spec* spec, int64_t overlap, const td_window_outputs* dev_out, int64_t rows_capacity,
                          void* d_counts, void* hip_stream);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and td_window_rows in one call: the ids stay on
 * the device.  Synchronous. */
int td_encode_batch_window_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                const td_rows_spec* spec, int64_t overlap, const td_window_outputs* host_out, int64_t rows_capacity,
                                int64_t* counts);

/* ---- label rows: a second stream placed beside the ids, in every row layout (td_*_labeled) -------------------------------------
 * A LABEL STREAM is a second int32 array src[n_tokens], index-aligned with ids (e.g. the labels of td_span_labels*).  The labeled
 * form of a row entry point places it by the very same placement as the ids into dst[rows_capacity * S], in the same pass: the
 * slot kernels resolve every slot's source index once and move both streams.  For every layout:
 *   a slot whose id row holds body id ids[i] holds src[i];
 *   a slot that holds the inserted BOS holds bos_value, the inserted EOS eos_value, a pad slot pad_value (any int32 each);
 *   with TD_ROWLAB_MASK_OVERLAP (TD_ROWS_WINDOWS only), body slot j < overlap of a window k > 0 holds pad_value instead of src[i]:
 *   these are the ids the window repeats, so every id of a document is trained in exactly one row.
 * Values in src are data: any int32, never checked.  src and dst are host or device memory, as the entry point's ids and out ids.
 * Spec errors are TD_E_INVALID with a message, before any launch and behind the counterpart's own argument checks: a value
 * outside int32, unknown flags, TD_ROWLAB_MASK_OVERLAP on another layout, src or dst NULL.
 * Each labeled entry point has the signature of its counterpart plus a trailing td_rows_labels.  Every other output equals the
 * counterpart's byte for byte; error codes, err_pos, the order of the checks and the synchronisation are the counterpart's
 * (td_pack_rows_labeled_device synchronises once, the other device forms not at all); where the counterpart writes nothing on an
 * error (capacity, bad offsets), nothing is written to dst either.
 * Without BOS / EOS, dst is what the counterpart makes of src in place of ids with pad_id = pad_value. */
#define TD_ROWLAB_MASK_OVERLAP 1   /* TD_ROWS_WINDOWS only */
typedef struct td_rows_labels {
    const int32_t* src;   /* host or device memory, as the entry point's ids */
    int32_t* dst;         /* like the entry point's out ids */
    int64_t bos_value;    /* any int32: what dst holds where the id row holds the inserted BOS */
    int64_t eos_value;    /* ... the inserted EOS */
    int64_t pad_value;    /* ... a pad slot */
    int64_t flags;
} td_rows_labels;
int td_make_rows_labeled(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                         const td_rows_spec* spec, int32_t* out_ids, int64_t rows_capacity, int32_t* out_positions, int32_t* out_aux,
                         int64_t* counts, const td_rows_labels* lab);
int td_make_rows_labeled_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                                const td_rows_spec* spec, void* d_out_ids, int64_t rows_capacity, void* d_positions, void* d_aux,
                                void* d_counts, void* hip_stream, const td_rows_labels* lab);
int td_pack_rows_labeled(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                         const td_rows_spec* spec, const td_pack_outputs* host_out, int64_t rows_capacity, int64_t* counts,
                         const td_rows_labels* lab);
int td_pack_rows_labeled_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                                const td_rows_spec* spec, const td_pack_outputs* dev_out, int64_t rows_capacity, int64_t* counts,
                                void* hip_stream, const td_rows_labels* lab);
int td_window_rows_labeled(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                           const td_rows_spec* spec, int64_t overlap, const td_window_outputs* host_out, int64_t rows_capacity,
                           int64_t* counts, const td_rows_labels* lab);
int td_window_rows_labeled_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                                  const td_rows_spec* spec, int64_t overlap, const td_window_outputs* dev_out, int64_t rows_capacity,
                                  void* d_counts, void* hip_stream, const td_rows_labels* lab);

/* ---- document selection: choose, reorder, repeat and length-filter encoded documents (td_select.hip) ---------------------------
 * Every call above consumes ids[n_tokens] + tok_offsets[n_docs + 1] "concatenated in document order".  This one changes the
 * order and the choice without leaving the device, and its output is again ids + tok_offsets: it composes with every row layout
 * and with the label stream.  A gather: no randomness is made here and no document is cut; the order is the caller's list, and
 * the result is a pure function of the inputs.
 *   L_d = tok_offsets[d + 1] - tok_offsets[d].
 *   sel[n_sel] (int64): document indices in the order the output is to have them.  Repeats are allowed (a document listed twice
 *   appears twice) and n_sel may exceed n_docs.  sel == NULL is the identity 0 .. n_docs - 1 and requires n_sel == n_docs.
 *   Entry i is KEPT iff min_len <= L_sel[i] and (max_len < 0 or L_sel[i] <= max_len).  K = the kept entries, i_0 < ... < i_{K-1}.
 *     out_docs[k] = sel[i_k]                                               int64, K written; the pointer may be NULL
 *     out_offsets[0] = 0, out_offsets[k + 1] = out_offsets[k] + L_out_docs[k]   int64, room for n_sel + 1, K + 1 written
 *     out_ids[out_offsets[k] + q] = ids[tok_offsets[out_docs[k]] + q]       int32, room for ids_capacity, T = out_offsets[K] written
 *     out_labels[...] = labels[...] by the same indices: an optional second int32 stream labels[n_tokens] (e.g. td_span_labels'),
 *                       both pointers NULL or both given; moved in the same pass by the same resolved source
 *     counts[4] (int64) = {K, T, entries dropped below min_len, entries dropped above max_len}; [0] + [2] + [3] = n_sel.
 *   Errors:
 *     a bad spec (min_len < 0, max_len < -1, 0 <= max_len < min_len, flags != 0) and sel == NULL with n_sel != n_docs:
 *       TD_E_INVALID before any launch;
 *     sel[i] outside [0, n_docs), or offsets of document sel[i] that are not 0 <= lo <= hi <= n_tokens: TD_E_INVALID with
 *       position i.  Only the offsets of listed documents are looked at; no id outside [0, n_tokens) is ever read;
 *     T > ids_capacity: TD_E_CAPACITY with counts[1] = T.
 *   On any error nothing is written to out_ids, out_labels, out_offsets or out_docs (the rule of the row calls).
 *   out_ids must not alias ids (nor out_labels labels): selecting in place is not supported. */
typedef struct td_select_spec {
    int64_t min_len; /* >= 0: listed documents with L < min_len are dropped */
    int64_t max_len; /* -1: no limit; otherwise >= min_len: listed documents with L > max_len are dropped */
    int64_t flags;   /* 0 */
} td_select_spec;

/* The contract's executable statement, on the host, from tok_offsets alone (no handle, no device): counts, and out_offsets
 * [n_sel + 1] and out_docs [n_sel] where not NULL.  Argument errors (a NULL tok_offsets / spec / counts, negative sizes, a bad
 * spec, sel == NULL with n_sel != n_docs) are TD_E_INVALID with counts[0] = -1; a bad entry i (sel[i] outside [0, n_docs), or
 * offsets of its document that are negative or decrease) is TD_E_INVALID with counts[0] = i.  Nothing else is written then. */
int td_select_plan(const int64_t* tok_offsets, int64_t n_docs, const int64_t* sel, int64_t n_sel, const td_select_spec* spec,
                   int64_t* counts, int64_t* out_offsets, int64_t* out_docs);
/* DEVICE buffers, asynchronously on hip_stream: no synchronisation and no read-back.  d_counts (4 int64) is device memory.
 * Errors surface through td_device_status: TD_E_INVALID with err_pos = a bad entry i, TD_E_CAPACITY with err_pos = T (and
 * counts[1] = T). */
int td_select_docs_device(td_tokenizer* t, const void* d_ids, const void* d_labels, int64_t n_tokens, const void* d_tok_offsets,
                          int64_t n_docs, const void* d_sel, int64_t n_sel, const td_select_spec* spec, void* d_out_ids,
                          void* d_out_labels, int64_t ids_capacity, void* d_out_offsets, void* d_out_docs, void* d_counts,
                          void* hip_stream);
/* Host buffers, synchronously.  tok_offsets is checked like every host entry point's offsets.  T is known on the host (the
 * plan): a capacity below it fails before any launch.  td_last_error names a bad entry's position. */
int td_select_docs(td_tokenizer* t, const int32_t* ids, const int32_t* labels, int64_t n_tokens, const int64_t* tok_offsets,
                   int64_t n_docs, const int64_t* sel, int64_t n_sel, const td_select_spec* spec, int32_t* out_ids,
                   int32_t* out_labels, int64_t ids_capacity, int64_t* out_offsets, int64_t* out_docs, int64_t* counts);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and td_select_docs in one call, "tokenize, then
 * drop what is too short": the ids stay on the device between the two.  sel indexes the documents of doc_offsets.  Synchronous. */
int td_encode_batch_select(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                           const int64_t* sel, int64_t n_sel, const td_select_spec* spec, int32_t* out_ids, int64_t ids_capacity,
                           int64_t* out_offsets, int64_t* out_docs, int64_t* counts);

/* ---- field joins: one example from several encoded fields (td_join.hip) --------------------------------------------------------
 * Fine-tuning data is several fields an example: prompt + completion, prompt + chosen / rejected, query + passage, chat turns.
 * Each field is a DOCUMENT of the stream; this call puts the K fields of an example into one output document, with literal ids
 * (the template: BOS, header markers, SEP, EOS) between them, per-field and per-example truncation, and a label and a type stream
 * written in the same pass.  The output is again ids + tok_offsets (+ labels, + types): it feeds the labeled row calls, the
 * selection, the counts and the n-gram matches unchanged.  Field text encoded with no special token allowed cannot spoof the
 * template, because the template never passes through text.
 *   Input.  K = spec.n_fields, 1 <= K <= TD_JOIN_MAX_FIELDS.  n_docs must be a multiple of K, n_ex = n_docs / K.  Field f of
 *   example x is document x * K + f; under TD_JOIN_FIELD_MAJOR it is document f * n_ex + x (two separately held batches, their
 *   buffers concatenated).  L_f = that document's length.
 *   Per field (td_join_field): before[n_before], 0 .. TD_JOIN_MAX_LITERAL literal ids written in front of the field's body;
 *   max_len, -1 or a cap >= 0 on the body; shrink_rank, 0 = never cut for the total, > 0 = may be cut; type_value, any int32;
 *   flags: TD_JOIN_KEEP_TAIL (a cut body keeps its LAST ids), TD_JOIN_TRAIN (body slots are trained), TD_JOIN_TRAIN_BEFORE (the
 *   field's literal slots are trained).
 *   Per spec: tail[n_tail], 0 .. 16 literal ids behind the last field; tail_type; max_total, -1 or >= 0; shrink, TD_JOIN_SHRINK_ORDER
 *   or TD_JOIN_SHRINK_LONGEST; ignore_index, any int32; flags: TD_JOIN_FIELD_MAJOR, TD_JOIN_TRAIN_TAIL.  Every literal id must be
 *   an id of the vocabulary, ordinary or special (else TD_E_BAD_TOKEN): the rule of bos_id / eos_id.
 *   Kept lengths c_f of one example, in this order:
 *     1. c_f = L_f, or min(L_f, max_len_f) where a cap is set.
 *     2. fixed = sum n_before_f + n_tail, need = fixed + sum c_f.  max_total < 0 or need <= max_total: the lengths are final.
 *     3. over = need - max_total.
 *        TD_JOIN_SHRINK_ORDER: the fields with shrink_rank > 0 by ascending rank, equal ranks by ascending field index; for each,
 *          cut = min(c_f, over), c_f -= cut, over -= cut.
 *        TD_JOIN_SHRINK_LONGEST: `over` times, one id is taken from the field with the largest c_f among those with shrink_rank > 0
 *          and c_f > 0, a tie going to the HIGHEST field index (Hugging Face's longest_first, which pops from the second of a tied
 *          pair); each step lowers `over` by one; it stops when no such field is left.  (Computed in closed form.)
 *     4. over > 0 still: the example does not fit and is DROPPED.  Otherwise it is kept, and it is TRUNCATED if any c_f < L_f.
 *   Output for the kept examples x_0 < ... < x_{E-1}:
 *     out ids of an example = before_0 body_0 before_1 body_1 ... before_{K-1} body_{K-1} tail, body_f = the first c_f ids of the
 *       field, or its last c_f under TD_JOIN_KEEP_TAIL                        int32, room for ids_capacity, T written
 *     offsets[E + 1], offsets[0] = 0                                          int64, room for n_ex + 1
 *     examples[E] = x_k                                                       int64, room for n_ex; may be NULL
 *     labels: the slot's id where its part is trained, ignore_index elsewhere  int32, as ids; may be NULL
 *     types: the field's type_value on its literals and body, tail_type on the tail   int32, as ids; may be NULL
 *     field_len[E * K] = the kept c_f (saturating at 2^31 - 1)                int32, room for n_ex * K; may be NULL
 *     counts[4] (int64) = {E, T = offsets[E], examples dropped, examples truncated}; [0] + [2] = n_ex.
 *     An example whose every part is empty is kept as an empty output document.
 *   Errors, by the rules of the selection and the row calls:
 *     before any launch, TD_E_INVALID with a message: a bad spec (K out of range, literal counts out of range, max_len < -1,
 *       max_total < -1, shrink_rank < 0, unknown shrink or flags, a value outside int32 where int32 is meant), n_docs % K != 0,
 *       ids of the output overlapping the input ids;
 *     offsets of a document that are not 0 <= lo <= hi <= n_tokens: TD_E_INVALID with position = the example.  No id outside
 *       [0, n_tokens) is ever read;
 *     T > ids_capacity: TD_E_CAPACITY with counts[1] = T.
 *   On any error nothing is written to any output but counts. */
#define TD_JOIN_MAX_FIELDS 8
#define TD_JOIN_MAX_LITERAL 16
#define TD_JOIN_KEEP_TAIL 1    /* td_join_field.flags */
#define TD_JOIN_TRAIN 2
#define TD_JOIN_TRAIN_BEFORE 4
#define TD_JOIN_FIELD_MAJOR 1  /* td_join_spec.flags */
#define TD_JOIN_TRAIN_TAIL 2
#define TD_JOIN_SHRINK_ORDER 0 /* td_join_spec.shrink */
#define TD_JOIN_SHRINK_LONGEST 1
typedef struct td_join_field {
    int64_t before[TD_JOIN_MAX_LITERAL];
    int64_t n_before;
    int64_t max_len;     /* -1: no cap */
    int64_t shrink_rank; /* 0: never cut for max_total */
    int64_t type_value;  /* int32 */
    int64_t flags;
} td_join_field;
typedef struct td_join_spec {
    int64_t n_fields;
    td_join_field fields[TD_JOIN_MAX_FIELDS];
    int64_t tail[TD_JOIN_MAX_LITERAL];
    int64_t n_tail;
    int64_t tail_type;    /* int32 */
    int64_t max_total;    /* -1: no limit */
    int64_t shrink;
    int64_t ignore_index; /* int32 */
    int64_t flags;
} td_join_spec;
/* Where a join writes: host pointers for td_join_fields / td_encode_batch_join, device pointers for td_join_fields_device. */
typedef struct td_join_outputs {
    void* ids;            /* int32[ids_capacity] */
    void* labels;         /* int32[ids_capacity] or NULL */
    void* types;          /* int32[ids_capacity] or NULL */
    int64_t ids_capacity;
    void* offsets;        /* int64[n_ex + 1] */
    void* examples;       /* int64[n_ex] or NULL */
    void* field_len;      /* int32[n_ex * K] or NULL */
} td_join_outputs;

/* The contract's executable statement, on the host, from tok_offsets and the spec alone (no handle, no device, so literal ids
 * are not looked up): counts, and out_offsets [n_ex + 1], out_examples [n_ex] and out_field_len [n_ex * K] where not NULL.  It
 * runs the truncation rule the kernels run.  Argument errors (NULL tok_offsets / spec / counts, a bad spec, n_docs % K != 0) are
 * TD_E_INVALID with counts[0] = -1; offsets of an example's document that are negative, decrease or exceed 2^59 are TD_E_INVALID
 * with counts[0] = the example.  Nothing else is written then. */
int td_join_plan(const int64_t* tok_offsets, int64_t n_docs, const td_join_spec* spec, int64_t* counts, int64_t* out_offsets,
                 int64_t* out_examples, int32_t* out_field_len);
/* DEVICE buffers, asynchronously on hip_stream: no synchronisation and no read-back.  d_counts (4 int64) is device memory.
 * Errors surface through td_device_status: TD_E_INVALID with err_pos = the example, TD_E_CAPACITY with err_pos = T (and
 * counts[1] = T). */
int td_join_fields_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                          const td_join_spec* spec, const td_join_outputs* d_out, void* d_counts, void* hip_stream);
/* Host buffers, synchronously.  tok_offsets is checked like every host entry point's offsets.  The plan is known on the host:
 * a capacity below T fails before any launch. */
int td_join_fields(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                   const td_join_spec* spec, const td_join_outputs* out, int64_t* counts);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and td_join_fields in one call: the ids stay
 * in the workspace between the two.  Field text cannot spoof the template: a field that contains the literal string of a
 * special token comes out as that string's ordinary ids, while the template's special arrives as its id.  Synchronous. */
int td_encode_batch_join(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                         const td_join_spec* spec, const td_join_outputs* out, int64_t* counts);

/* ---- loss labels: train only inside marked id spans (td_labels.hip) ----------------------------------------------------------
 * ids + per-document token offsets -> labels[i] = ids[i] where the loss applies, ignore_index everywhere else.  The rule knows
 * no chat template: a span is opened by an opener id SEQUENCE (e.g. the three ids of <|header_start|>assistant<|header_end|>)
 * and closed by a closer ID (e.g. <|eot|>, <|eom|>).
 *
 * Per document [a, z) = [tok_offsets[d], tok_offsets[d + 1]):
 *   open event at q    some opener o of length k has ids[q-k+1 .. q] == o with q-k+1 >= a (a match never reaches across a
 *                      document start);
 *   close event at q   ids[q] is a closer.  No opener may contain a closer, so no position is both kinds of event;
 *   inside(i), a <= i <= z: the last event at a position in [a, i) is an open event (no event: false);
 *   trained(i) = inside(i) && (!close(i) || TD_LABELS_TRAIN_CLOSE).
 * So the header ids are not trained (the opener that starts a span lies in front of it), nor anything outside spans; an opener
 * while already inside is content; a closer while outside has no effect; a document that ends inside is "unterminated".
 * This is the obvious sequential two-state walk over every document.
 *
 * Outputs:
 *   labels[i] = trained(i) ? ids[i] : ignore_index                                   (int32, required)
 *   mask[i] = trained(i)                                                             (uint8, optional)
 *   trained_offsets[n_docs + 1]: the trained ids in front of every document start, the total last; its differences are the
 *                                per-document trained counts                         (int64, optional)
 *   counts[4] = {trained ids, spans (open events at q with !inside(q)), unterminated documents, 0}   (int64, required)
 * Slots at or above tok_offsets[n_docs] are not written.
 *
 * Spec errors are TD_E_INVALID with a message, before any launch: n_open outside 1..8, an open_len outside 1..8, n_close
 * outside 0..16, a negative spec id, a closer inside an opener, ignore_index outside int32, unknown flags.  Ids in the DATA are
 * not checked against the vocabulary: a negative or out-of-range id matches nothing. */
#define TD_LABELS_MAX_OPEN 8      /* opener sequences */
#define TD_LABELS_MAX_OPEN_LEN 8  /* ids per opener */
#define TD_LABELS_MAX_CLOSE 16
#define TD_LABELS_TRAIN_CLOSE 1   /* flags: a closer that ends a span is itself trained (the model must learn to stop) */
typedef struct td_labels_spec {
    int64_t n_open;
    int64_t open_len[TD_LABELS_MAX_OPEN];
    int32_t open_ids[TD_LABELS_MAX_OPEN][TD_LABELS_MAX_OPEN_LEN];
    int64_t n_close;
    int32_t close_ids[TD_LABELS_MAX_CLOSE];
    int64_t ignore_index; /* any int32, e.g. -100 */
    int64_t flags;
} td_labels_spec;

/* Device buffers, asynchronously on hip_stream (never the null stream's work of the library itself; no synchronisation, no
 * read-back).  d_mask and d_trained_offsets may be NULL.  tok_offsets that do not start at 0, decrease, are negative or end
 * above n_tokens raise TD_E_INVALID through td_device_status with err_pos = the first such document found; then nothing is
 * written to any output and no id outside [0, n_tokens) is read. */
int td_span_labels_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                          const td_labels_spec* spec, void* d_labels, void* d_mask, void* d_trained_offsets, void* d_counts,
                          void* hip_stream);
/* Host buffers, synchronous; tok_offsets are checked like every host entry point's.  mask and trained_offsets may be NULL. */
int td_span_labels(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                   const td_labels_spec* spec, int32_t* labels, uint8_t* mask, int64_t* trained_offsets, int64_t* counts);
/* td_encode_batch_with_special_strs (TD_MODE_ENCODE; the same ids and offsets) and td_span_labels in one call, from chat text
 * to ids + labels: where the encode leaves its ids on the device they are labelled there.  out_labels (and out_mask) have
 * room for out_capacity entries.  *n_tokens = ids needed (also on TD_E_CAPACITY).  Synchronous. */
int td_encode_batch_span_labels(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                const td_labels_spec* spec, int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets,
                                int32_t* out_labels, uint8_t* out_mask, int64_t* out_trained_offsets, int64_t* counts,
                                int64_t* n_tokens);

/* From chat text to trainer-ready (input_ids, labels) rows in one call: td_encode_batch_span_labels followed by the labeled row
 * call of rspec->layout (td_make_rows_labeled / td_pack_rows_labeled / td_window_rows_labeled; overlap: TD_ROWS_WINDOWS), with the
 * labels as the label stream.  Ids and labels stay on the device between the steps.  lab gives bos_value, eos_value, pad_value
 * and flags; its src and dst are ignored.  host_out: fields that the layout does not have must be NULL (TD_E_INVALID).
 * row_counts[4] are the row call's counts (also on TD_E_CAPACITY: [0] = the rows needed), label_counts[4] the labels'.
 * Synchronous. */
typedef struct td_label_rows_outputs {
    int32_t* ids;          /* int32 [rows * S] */
    int32_t* labels;       /* int32 [rows * S] */
    int32_t* positions;    /* optional */
    int32_t* aux;          /* optional: CONCAT cu_seqlens / PAD lengths / BESTFIT cu_seqlens */
    int32_t* row_lengths;  /* optional: BESTFIT, WINDOWS */
    int64_t* seg_docs;     /* optional: BESTFIT */
    int64_t* row_docs;     /* optional: WINDOWS */
    int64_t* row_starts;   /* optional: WINDOWS */
} td_label_rows_outputs;
int td_encode_batch_span_label_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                    const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                    const td_labels_spec* lspec, const td_rows_spec* rspec, int64_t overlap, const td_rows_labels* lab,
                                    const td_label_rows_outputs* host_out, int64_t rows_capacity, int64_t* row_counts,
                                    int64_t* label_counts);

/* ---- loss labels from byte ranges: train only on marked text ranges (td_ranges.hip) -------------------------------------------
 * For data whose trained regions are known as offsets into the TEXT (plain-text templates, prompt / completion pairs, field
 * values of tool traces), where td_labels_spec's id events do not exist.  Inputs beside ids[n_tokens] and tok_offsets[n_docs + 1]:
 *   range_offsets[n_docs + 1] (int64): the first range of every document; starts at 0, never decreases, ends at n_ranges;
 *   ranges[n_ranges][2] (int64, interleaved begin, end): byte offsets RELATIVE TO THE DOCUMENT'S FIRST BYTE, half-open.
 * Per document the ranges must satisfy 0 <= begin <= end and be sorted and disjoint: begin[r + 1] >= end[r].  Touching ranges
 * and empty ranges are legal; an empty range marks nothing.
 *
 * Byte p of document d is MARKED iff some range of d has begin <= p < end.  Id i of d occupies the bytes [s_i, e_i),
 * e_i = s_i + len(ids[i]) (the length of the id's bytes in the vocabulary, special tokens included); m_i is the number of marked
 * bytes among them.  trained(i) by td_range_spec.rule:
 *   TD_RANGE_OVERLAP   m_i > 0
 *   TD_RANGE_INSIDE    m_i == e_i - s_i
 *   TD_RANGE_START     byte s_i is marked
 * Because the rule is by bytes, two touching ranges behave as one and empty ranges need no special case.
 *
 * Outputs, as td_span_labels':
 *   labels[i] = trained(i) ? ids[i] : ignore_index                                   (int32, required)
 *   mask[i] = trained(i)                                                             (uint8, optional)
 *   trained_offsets[n_docs + 1]: the trained ids in front of every document start, the total last   (int64, optional)
 *   counts[4] = {trained ids, partially marked ids (0 < m_i < e_i - s_i: they straddle an edge of a range),
 *                marked bytes (the sum of end - begin), 0}                           (int64, required)
 * Slots at or above tok_offsets[n_docs] are not written.
 *
 * Where s_i comes from:
 *   starts == NULL   the COVERED rule of td_token_starts: every document's bytes are its ids' bytes concatenated, s_i is the sum of
 *                    the lengths in front of i in its document.  The starts are scanned on the fly and never stored.  An id
 *                    outside the vocabulary is TD_E_BAD_TOKEN with its index (the lowest), as in td_token_starts.  A range that
 *                    ends beyond the document's covered bytes is TD_E_INVALID with err_pos = the global index of the first such
 *                    range (the lowest); a document without ids may have no range with end > 0.
 *   starts != NULL   int64 byte starts, one per id, as td_encode_*_with_starts produce them (TD_UNIT_BYTES; they do not decrease
 *                    inside a document): the way in for generic patterns that skip text.  len still comes from the vocabulary (an
 *                    id outside it: TD_E_BAD_TOKEN); the upper bound of the ranges is not checked, the document's length is unknown.
 *
 * Errors.  Spec errors (unknown rule, flags != 0, ignore_index outside int32) are TD_E_INVALID with a message, before any launch.
 * tok_offsets or range_offsets that do not start at 0, decrease, are negative or end above n_tokens / differ from n_ranges at the
 * end: TD_E_INVALID with err_pos = the document.  A range that is negative, reversed, or begins in front of the end of the one
 * before it in its document: TD_E_INVALID with err_pos = the global range index, the lowest.  These structural errors are found
 * before anything is written: no output is touched.  The covered form finds a range beyond its document during the labelling pass:
 * the outputs are then unspecified and the error is reported. */
#define TD_RANGE_OVERLAP 0
#define TD_RANGE_INSIDE 1
#define TD_RANGE_START 2
typedef struct td_range_spec {
    int64_t rule;         /* TD_RANGE_* */
    int64_t ignore_index; /* any int32, e.g. -100 */
    int64_t flags;        /* 0 */
} td_range_spec;

/* The structural checks alone, on the host (no handle, no device): range_offsets, then every range in order.  doc_lens[n_docs]
 * (may be NULL): the documents' byte lengths, a range may not end above its document's.  counts[2] = {non-empty ranges, marked
 * bytes}.  TD_E_INVALID with *bad = the first bad document (range_offsets) or the first bad global range index; *bad = -1 for a
 * NULL argument or n_docs < 0.  counts and bad may be NULL. */
int td_range_plan(const int64_t* range_offsets, const int64_t* ranges, int64_t n_docs, const int64_t* doc_lens, int64_t* counts,
                  int64_t* bad);
/* Device buffers, asynchronously on hip_stream (no synchronisation, no read-back); errors through td_device_status.  d_starts,
 * d_mask and d_trained_offsets may be NULL; d_ranges must be 8-byte aligned. */
int td_range_labels_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                           const void* d_starts, const void* d_range_offsets, const void* d_ranges, int64_t n_ranges,
                           const td_range_spec* spec, void* d_labels, void* d_mask, void* d_trained_offsets, void* d_counts,
                           void* hip_stream);
/* Host buffers, synchronous; the offsets and the ranges' order are checked on the host first (td_range_plan).  starts, mask and
 * trained_offsets may be NULL. */
int td_range_labels(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                    const int64_t* starts, const int64_t* range_offsets, const int64_t* ranges, const td_range_spec* spec,
                    int32_t* labels, uint8_t* mask, int64_t* trained_offsets, int64_t* counts);
/* td_encode_batch_with_special_strs (the same ids and offsets) and the covered form in one call, from text and byte ranges into it
 * to ids + labels: where the encode leaves its ids on the device they are labelled there.  Range ends are checked against
 * doc_offsets as well (td_range_plan with the documents' lengths).  A document whose ids cover fewer bytes than it has (a generic
 * split pattern that skipped text) fails with TD_E_INVALID: use td_encode_batch_with_starts and the explicit-starts form.
 * out_labels (and out_mask) have room for out_capacity entries.  *n_tokens = ids needed (also on TD_E_CAPACITY).  Synchronous. */
int td_encode_batch_range_labels(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                 const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                 const int64_t* range_offsets, const int64_t* ranges, const td_range_spec* spec, int32_t* out_tokens,
                                 int64_t out_capacity, int64_t* out_offsets, int32_t* out_labels, uint8_t* out_mask,
                                 int64_t* out_trained_offsets, int64_t* counts, int64_t* n_tokens);
/* td_encode_batch_span_label_rows with byte ranges in place of id spans: td_encode_batch_range_labels followed by the labeled row
 * call of rspec->layout.  Ids and labels stay on the device between the steps; everything else as there. */
int td_encode_batch_range_label_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                     const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                     const int64_t* range_offsets, const int64_t* ranges, const td_range_spec* rgspec,
                                     const td_rows_spec* rspec, int64_t overlap, const td_rows_labels* lab,
                                     const td_label_rows_outputs* host_out, int64_t rows_capacity, int64_t* row_counts,
                                     int64_t* label_counts);

/* ---- token counts: histograms of ids per document group (td_counts.hip) ----------------------------------------------------------
 * What is in the ids a call made: counts[g * n_bins + v] = the visited positions of group g whose value is v, without copying the
 * ids to the host.  ids[n_tokens] (int32) is any stream aligned with ids: passing the labels of td_span_labels / td_range_labels
 * gives the histogram of the TRAINED tokens, their negative ignore_index falls out by the rule below.
 *   n_groups == 1: positions [0, n_tokens) are visited; tok_offsets, n_docs and doc_group are ignored and may be NULL / 0.
 *   n_groups > 1:  tok_offsets[n_docs + 1] (int64) and doc_group[n_docs] (int32) are required; positions [tok_offsets[0],
 *                  tok_offsets[n_docs]) are visited, position i belongs to the document d with tok_offsets[d] <= i < tok_offsets[d + 1]
 *                  and to group doc_group[d] (a source, a language, a split).
 *   counts[n_groups * n_bins] (int64, row-major by group).  Without TD_COUNTS_ACCUMULATE it is zeroed first; with it the call adds to
 *                  what is there (several calls, several shards).
 *   info[4] (int64), always overwritten: every visited position falls into exactly one of, in this order of precedence,
 *     info[3] bad_group  its document's group is outside [0, n_groups)
 *     info[1] negative   v < 0
 *     info[2] too_large  v >= n_bins
 *     info[0] counted    added to counts
 *   so the four add up to the visited positions.  A value is never an error and never moves a write outside counts.  Integer sums
 *   are exact in any order: results are bitwise reproducible.
 *   Errors:
 *     a bad spec (n_bins < 1, n_groups < 1, n_groups * n_bins > 2^28, flags other than TD_COUNTS_ACCUMULATE, n_groups > 1 with a
 *       NULL tok_offsets or doc_group): TD_E_INVALID before any launch;
 *     host forms: tok_offsets (where n_groups > 1) are checked like the row calls' offsets, and a doc_group[d] outside
 *       [0, n_groups) is TD_E_INVALID naming d; both before any launch, counts untouched;
 *     device form: a document WITH visited positions whose group is bad raises TD_E_INVALID with err_pos = d through
 *       td_device_status, and info[3] tells how many positions such documents held; the other documents are counted.  Offsets that
 *       decrease, begin below 0 or end above n_tokens raise TD_E_INVALID where the kernel meets them; counts is then unspecified,
 *       but nothing outside ids[0, n_tokens) is read and nothing outside counts / info is written. */
#define TD_COUNTS_ACCUMULATE 1
typedef struct td_counts_spec {
    int64_t n_bins;   /* >= 1: values v with 0 <= v < n_bins are counted */
    int64_t n_groups; /* >= 1; n_groups * n_bins <= 2^28 */
    int64_t flags;    /* 0 or TD_COUNTS_ACCUMULATE */
} td_counts_spec;

/* The contract's executable statement, on the host (no handle, no device).  tok_offsets (n_groups > 1) must be non-negative and
 * non-decreasing and end at or below n_tokens; tok_offsets[0] may be above 0.  Argument errors (a NULL spec / counts / info, a bad
 * spec, negative sizes, bad offsets, NULL ids with positions to visit) are TD_E_INVALID with info[0] = -1; a doc_group[d] outside
 * [0, n_groups) is TD_E_INVALID with info[0] = d, the lowest.  counts is untouched then. */
int td_token_counts_host(const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, const int32_t* doc_group,
                         const td_counts_spec* spec, int64_t* counts, int64_t* info);
/* DEVICE buffers, asynchronously on hip_stream: no synchronisation and no read-back; the zeroing of d_counts, when asked for, is
 * enqueued on the same stream.  d_counts (n_groups * n_bins int64) and d_info (4 int64) are device memory, 8-byte aligned. */
int td_token_counts_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                           const void* d_doc_group, const td_counts_spec* spec, void* d_counts, void* d_info, void* hip_stream);
/* Host buffers, synchronously.  With TD_COUNTS_ACCUMULATE the device's result is added to the caller's array on the host. */
int td_token_counts(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                    const int32_t* doc_group, const td_counts_spec* spec, int64_t* counts, int64_t* info);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and the counts in one call, "statistics at encode
 * speed": the ids never leave the device, only counts, info and *n_tokens_out (the ids made; may be NULL) come back.  doc_group
 * (n_groups > 1) indexes the documents of doc_offsets.  Synchronous. */
int td_encode_batch_token_counts(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                 const int32_t* doc_group, const td_counts_spec* spec, int64_t* counts, int64_t* info,
                                 int64_t* n_tokens_out);

/* ---- n-gram matches: listed id sequences found in documents (td_ngrams.hip) ----------------------------------------------------------
 * "Does this document contain any of these known token sequences?" without copying the ids to the host: benchmark decontamination
 * (every 13-gram of an evaluation set), phrase blocklists, counting canary strings or tool-call markers.
 * A SET holds n_pats id sequences ("patterns"): pat_ids (int32, flat) and pat_offsets[n_pats + 1] (int64, from 0, non-decreasing).
 *   Every pattern's length k is in 1 .. TD_NGRAM_MAX_LEN, at most TD_NGRAM_MAX_LENGTHS distinct lengths occur, ids are >= 0, n_pats is
 *   in 1 .. 2^24 and pat_offsets[n_pats] at most 2^28; anything else is TD_E_INVALID with a message, at creation.  Equal sequences
 *   may repeat in the list: they are ONE pattern, known by the lowest of their indices.
 * Per document [a, z) = [tok_offsets[d], tok_offsets[d + 1]):
 *   an OCCURRENCE is a pair (q, k) with a <= q, q + k <= z and ids[q .. q + k) equal to some pattern of length k; it never reaches
 *   across a document boundary.  Overlapping and nested occurrences all count: [7,7] occurs three times in 7,7,7,7.
 *   covered(i) holds when some occurrence (q, k) has q <= i < q + k.
 *   The ids of the data are not checked against a vocabulary: negative or huge values match nothing, so label streams may be searched.
 * Outputs, all optional (NULL) except counts; slots at or above tok_offsets[n_docs] are never written:
 *   cover[i]   (uint8)  covered(i)
 *   labels[i]  (int32, IN PLACE) set to ignore_index where covered(i) holds, every other slot is not stored to: the caller passes a
 *              copy of the ids or an existing label stream (never the buffer the call reads as ids)
 *   doc_stats[d][2] (int64) = {occurrences starting in d, covered ids of d}
 *   pattern_counts[n_pats] (int64) the occurrences of every pattern; a repeated sequence counts under its lowest index, its other
 *              indices stay 0.  Zeroed first, or added to under TD_NGRAM_ACCUMULATE.
 *   counts[4] (int64) = {occurrences, covered ids, documents with at least one occurrence, 0}
 * The lookup hashes a window only to FIND a candidate and compares the ids before it reports anything: the results are a function of
 * the inputs alone (not of the hash, the table size, TD_OPT_NGRAM_TAG_BITS or the launch shape), and all sums are integer sums:
 * bitwise reproducible.
 * Out of scope: a list of match positions (its order would depend on scheduling), patterns with wildcards, near-duplicate
 * detection (its signatures: td_minhash* below), sets that span several devices. */
#define TD_NGRAM_MAX_LEN 64
#define TD_NGRAM_MAX_LENGTHS 8
#define TD_NGRAM_ACCUMULATE 1
typedef struct td_ngram_spec {
    int64_t ignore_index; /* what labels[i] becomes where covered(i) holds; an int32 */
    int64_t flags;        /* 0 or TD_NGRAM_ACCUMULATE */
} td_ngram_spec;
typedef struct td_ngram_set td_ngram_set;

/* Validates and de-duplicates the list, builds the lookup table on the host and uploads it to t's device (synchronous).  The set is
 * immutable afterwards: any handle on that device, td_clone's included, may use it on any stream, concurrently.  It does not keep t.
 * Errors: TD_E_INVALID with a message in td_last_error(t). */
int td_ngram_set_create(td_tokenizer* t, const int32_t* pat_ids, const int64_t* pat_offsets, int64_t n_pats, td_ngram_set** out);
/* Frees the set's device memory at once, like hipFree: the caller must have finished (synchronised) the work that uses the set. */
void td_ngram_set_destroy(td_ngram_set* set);
#define TD_NGRAM_INFO_PATTERNS 1     /* the patterns given */
#define TD_NGRAM_INFO_DISTINCT 2     /* the distinct ones */
#define TD_NGRAM_INFO_LENGTHS 3      /* the distinct lengths */
#define TD_NGRAM_INFO_MAX_LEN 4      /* the longest */
#define TD_NGRAM_INFO_SLOTS 5        /* the table's slots: a power of two, at least twice the distinct patterns */
#define TD_NGRAM_INFO_MAX_PROBE 6    /* the longest distance between a pattern's first slot and its own: what bounds every lookup */
#define TD_NGRAM_INFO_DEVICE_BYTES 7 /* the device memory the set holds */
int64_t td_ngram_set_info(const td_ngram_set* set, int what); /* -1: no such value */

/* The contract's executable statement, on the host (no handle, no device, no set: the list itself).  tok_offsets must start at 0, be
 * non-decreasing and end at or below n_tokens.  Argument errors (a bad list, bad offsets, a bad spec, NULL counts, NULL ids with ids to
 * visit) are TD_E_INVALID and nothing is written. */
int td_ngram_matches_host(const int32_t* pat_ids, const int64_t* pat_offsets, int64_t n_pats, const int32_t* ids, int64_t n_tokens,
                          const int64_t* tok_offsets, int64_t n_docs, const td_ngram_spec* spec, uint8_t* cover, int32_t* labels,
                          int64_t* doc_stats, int64_t* pattern_counts, int64_t* counts);
/* DEVICE buffers, asynchronously on hip_stream: no synchronisation and no read-back; the zeroing of the outputs is part of the
 * launches.  d_doc_stats, d_pattern_counts and d_counts are 8-byte aligned.  Offsets that do not start at 0, decrease, are negative
 * or end above n_tokens raise TD_E_INVALID through td_device_status with err_pos = the lowest such document, and then NOTHING is
 * written to any output.  A bad spec (unknown flags, an ignore_index outside int32) and a set of another device are TD_E_INVALID
 * before any launch. */
int td_ngram_matches_device(td_tokenizer* t, const td_ngram_set* set, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets,
                            int64_t n_docs, const td_ngram_spec* spec, void* d_cover, void* d_labels, void* d_doc_stats,
                            void* d_pattern_counts, void* d_counts, void* hip_stream);
/* Host buffers, synchronously; the offsets are checked like every host entry point's, before any launch.  labels is read and written. */
int td_ngram_matches(td_tokenizer* t, const td_ngram_set* set, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets,
                     int64_t n_docs, const td_ngram_spec* spec, uint8_t* cover, int32_t* labels, int64_t* doc_stats,
                     int64_t* pattern_counts, int64_t* counts);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and the matches in one call: the ids never leave
 * the device, only doc_stats[n_docs][2], pattern_counts (both may be NULL), counts and *n_tokens_out (the ids made; may be NULL) come
 * back.  Synchronous. */
int td_encode_batch_ngram_matches(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                  const td_ngram_set* set, const td_ngram_spec* spec, int64_t* doc_stats, int64_t* pattern_counts,
                                  int64_t* counts, int64_t* n_tokens_out);

/* ---- MinHash signatures and LSH band keys per document (td_minhash.hip) ----------------------------------------------------------------
 * What near-duplicate detection needs from the tokenizer's side, without copying the ids to the host: a signature per document over
 * its id shingles, and optionally the band keys that bucket documents into candidate groups.  Both are a pure function of ONE
 * document, so they compose across batches, calls and ranks; the clustering, which is global and a matter of policy, is the caller's.
 * Inputs: ids (int32), tok_offsets[n_docs + 1] (int64: from 0, non-decreasing, ending at or below n_tokens, as for td_ngram_matches*)
 * and a spec {k, num_perm, seed, bands, rows, flags}.  Per document [a, z) = [tok_offsets[d], tok_offsets[d + 1]), L = z - a:
 *   SHINGLES     L >= k: the L - k + 1 windows of k consecutive ids; none reaches across a document boundary.  1 <= L < k: ONE
 *                shingle, the whole document, hashed with its own length L.  L = 0: none.
 *   SHINGLE HASH 32 bits, x = finish(poly(window), len) with len = k or L: the n-gram matches' window hash, the library's only one.
 *                poly: h = 0, then h = h * 0x9E3779B1 + id over the window's ids as uint32 bit patterns, modulo 2^32.  finish:
 *                x = h + len * 0x7FEB352D; x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16.
 *                The ids are not checked against a vocabulary: label streams (-100 and all) may be sketched.
 *   PERMUTATIONS mix64(z), the splitmix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *                z ^= z >> 31.  With G = 0x9E3779B97F4A7C15 and j in 0 .. num_perm: a_j = mix64(seed + (2j + 1) G) | 1,
 *                b_j = mix64(seed + (2j + 2) G), h_j(x) = (uint32)((a_j * (uint64)x + b_j) >> 32), arithmetic modulo 2^64:
 *                multiply-add-shift, strongly universal for 32-bit keys (the strength class of (a x + b) mod p).
 *                td_minhash_params gives a_j and b_j, so another system can reproduce the family.
 *   SIGNATURE    sig[d][j] (uint32, [n_docs][num_perm]) = the minimum over d's shingles of h_j(x); 0xFFFFFFFF for a document with no id.
 *   BAND KEYS    optional (bands >= 1, rows >= 1, bands * rows <= num_perm): key[d][b] (uint64, [n_docs][bands]) = h after
 *                h = mix64(b + 1), then h = mix64(h ^ sig[d][j]) for j = b * rows .. (b + 1) * rows.  Equal keys in the same band
 *                mean "candidate pair".  Documents with no id all share their keys: drop them by counts or by their lengths.
 *   counts[4] (int64) = {shingles hashed, documents with no id, documents of 1 .. k - 1 ids (one short shingle each), 0}
 * Limits: k in 1 .. TD_NGRAM_MAX_LEN, num_perm in 1 .. TD_MINHASH_MAX_PERM, bands >= 0 (0: no keys; rows is then ignored), flags == 0,
 * band_keys not NULL when bands >= 1; anything else is TD_E_INVALID with a message, before any launch.
 * The result is a function of the inputs alone: a minimum does not depend on the order of its operands, so it is bitwise
 * reproducible whatever the launch shape or the scheduling is.
 * Out of scope: clustering and keep lists, signatures merged across calls (np.minimum of two does it), weighted or b-bit MinHash,
 * anything that makes the device decide which duplicate survives. */
#define TD_MINHASH_MAX_PERM 1024
typedef struct td_minhash_spec {
    int64_t k;        /* ids a shingle */
    int64_t num_perm; /* permutations: the signature's length */
    uint64_t seed;    /* of the family */
    int64_t bands;    /* 0: no band keys */
    int64_t rows;     /* signature entries a band */
    int64_t flags;    /* 0 */
} td_minhash_spec;
/* a[j], b[j] for j in 0 .. num_perm (no handle, no device).  TD_E_INVALID: num_perm outside 1 .. TD_MINHASH_MAX_PERM, a NULL array. */
int td_minhash_params(uint64_t seed, int64_t num_perm, uint64_t* a, uint64_t* b);
/* The contract's executable statement, on the host (no handle, no device).  Argument errors (bad offsets, a bad spec, NULL counts,
 * NULL sig with documents, NULL ids with ids to visit) are TD_E_INVALID and nothing is written. */
int td_minhash_host(const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, const td_minhash_spec* spec,
                    uint32_t* sig, uint64_t* band_keys, int64_t* counts);
/* DEVICE buffers, asynchronously on hip_stream: no synchronisation and no read-back; filling d_sig and zeroing d_counts is part of
 * the launches.  hip_stream is a stream of the caller's, never the null stream (TD_E_INVALID).  d_band_keys and d_counts are 8-byte
 * aligned, d_sig 4-byte.  Offsets that do not start at 0, decrease, are negative or end above n_tokens raise TD_E_INVALID through
 * td_device_status with err_pos = the lowest such document, and then NOTHING is written to any output.  The handle keeps the table of
 * (a_j, b_j) for the last (seed, num_perm): a call with another pair rebuilds it first, by a small kernel on hip_stream. */
int td_minhash_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                      const td_minhash_spec* spec, void* d_sig, void* d_band_keys, void* d_counts, void* hip_stream);
/* Host buffers, synchronously; the offsets are checked like every host entry point's, before any launch. */
int td_minhash(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, const td_minhash_spec* spec,
               uint32_t* sig, uint64_t* band_keys, int64_t* counts);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY, no allowed special tokens) and the signatures in one call: the ids never leave
 * the device, only sig, band_keys (NULL with bands == 0), counts and *n_tokens_out (the ids made; may be NULL) come back.  Synchronous. */
int td_encode_batch_minhash(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                            const td_minhash_spec* spec, uint32_t* sig, uint64_t* band_keys, int64_t* counts, int64_t* n_tokens_out);

/* ---- Unicode NFC normalisation (td_nfc.hip) ---------------------------------------------------------------------------------------------
 * The Qwen2 / Qwen2.5 / Qwen3 tokenizers normalise to NFC in front of their split pattern; the other supported families do not
 * normalise.  Text + doc_offsets[n_docs + 1] (int64: from 0, non-decreasing, ending at or below n_bytes) -> flags[d] (uint8: 0 = the
 * document is PROVEN to be its own NFC, 1 = not proven), and the normalised text + out_doc_offsets[n_docs + 1], which every
 * td_encode_* entry point takes as it stands.  The tables are generated from one Unicode version, which td_nfc_info reports; host and
 * device compile the same statement of the rule (td_nfc_args.h), so they cannot disagree.
 *   UNITS      At byte p of a document, a well-formed UTF-8 sequence (Unicode Table 3-7: no overlong form, no surrogate, nothing above
 *              U+10FFFF) that starts there and ends inside the document is a code point.  Otherwise byte p alone is an OPAQUE unit: it is
 *              copied unchanged, composes with nothing, and nothing is reordered across it.  No sequence reaches across a document
 *              boundary.
 *   BOUNDARY   A unit that is opaque, the first of its document, or a code point with ccc == 0 and NFC_Quick_Check == Yes.  A SEGMENT
 *              runs from a boundary to the next; documents and segments normalise independently.  Every code point that is no boundary
 *              is >= U+0300, so every unit led by a byte below 0xCC is a boundary.
 *   SEGMENT    UAX #15: canonical decomposition (at most 4 code points, Hangul by arithmetic), non-starters ordered stably by ccc, then
 *              composition: a mark composes with the current starter iff the pair is a primary composite and no kept unit with
 *              ccc == 0 or ccc >= its own lies between (Hangul LV, LVT by arithmetic; composition exclusions are no primary composites).
 *              Any length is handled.
 *   PROVEN     A stretch is proven NFC when every code point in it is Quick_Check Yes and ccc never decreases inside a run of
 *              non-starters.  A proven segment is copied; flags[d] == 1 iff document d holds a code point that is not Quick_Check Yes or
 *              a non-starter whose ccc is below that of the code point right in front of it.  Not proven does not mean changed (a Maybe
 *              with nothing to compose with).
 *   counts[8]  (int64) {output bytes needed, documents not proven, documents changed, segments rewritten (the segments not proven),
 *              code points in them, opaque bytes, the longest segment in code points, 0}.  [5] and [6] are over the whole text, proven
 *              or not (ASCII alone: 0 and 1).  td_nfc_check_device counts [1] alone, the rest is 0: the proof decodes nothing below
 *              0xCC.  So does td_encode_batch_nfc when no document is flagged: {n_bytes, 0, 0, 0, 0, 0, 0, 0}, [5] and [6] NOT counted.
 *   COST       A segment is normalised by one lane, in time linear in its length times the distinct ccc values in it: a document that is
 *              one run of millions of combining marks is rewritten correctly, by a single lane, and holds its call up accordingly.
 *   SIZES      The output is at most 3 x the input in bytes (U+1D1C0 reaches it): a capacity of 3 * n_bytes always fits.  An
 *              output that does not fit is TD_E_CAPACITY (position: the bytes needed, also in counts[0]); no byte of `out` is written.
 *              Bytes behind the last document are not copied.  changed[d] (uint8) = 1 iff the document's bytes differ.
 * Argument errors are TD_E_INVALID before any launch: offsets on the host that do not start at 0 or decrease, a NULL stream, an
 * output that overlaps the text.  Out of scope: NFD, NFKC, NFKD (the property word has five spare bits), a map from normalised bytes
 * back to source bytes, Unicode versions other than the tables'. */
#define TD_NFC_INFO_UNICODE_VERSION 0 /* major * 10000 + minor * 100 + patch */
#define TD_NFC_INFO_TABLE_BYTES 1
int64_t td_nfc_info(int what); /* -1: no such value */
/* The contract's executable statement, on the host (no handle, no device).  out may be NULL with out_capacity == 0: out_doc_offsets,
 * flags, changed (each may be NULL) and counts alone.  Argument errors write nothing. */
int td_nfc_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, uint8_t* out, int64_t out_capacity,
                int64_t* out_doc_offsets, uint8_t* flags, uint8_t* changed, int64_t* counts);
/* DEVICE buffers, asynchronously on hip_stream (never the null stream): no synchronisation and no read-back.  d_doc_offsets, d_counts
 * and d_out_doc_offsets are 8-byte aligned; d_text needs no alignment.  Offsets that do not start at 0, decrease, are negative or end
 * above n_bytes raise TD_E_INVALID through td_device_status with err_pos = the lowest such document, and then NOTHING is written. */
int td_nfc_check_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                        void* d_flags, void* d_counts, void* hip_stream);
/* d_changed may be NULL.  TD_E_CAPACITY surfaces through td_device_status; d_counts is complete then, d_out and d_out_doc_offsets are
 * not written. */
int td_nfc_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                  void* d_out, int64_t out_capacity, void* d_out_doc_offsets, void* d_changed, void* d_counts, void* hip_stream);
/* Host buffers, synchronously; td_nfc_host's arguments behind the handle. */
int td_nfc(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, uint8_t* out, int64_t out_capacity,
           int64_t* out_doc_offsets, uint8_t* flags, uint8_t* changed, int64_t* counts);
/* Upload, check, and td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY) of the ORIGINAL device buffer when no document is flagged;
 * otherwise the text is normalised into the handle's workspace and that is encoded.  out_tok_offsets[n_docs + 1], and everything later
 * computed from byte positions, refer to the NORMALISED text, which comes back on request: norm_text (may be NULL with norm_capacity
 * 0), norm_doc_offsets and changed (may be NULL).  When nothing changed the normalised text is the input.  counts: as td_nfc gives
 * them when a document is flagged, the check's otherwise (counts[8] above).  Synchronous. */
int td_encode_batch_nfc(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                        int32_t* out_ids, int64_t ids_capacity, int64_t* out_tok_offsets,
                        uint8_t* norm_text, int64_t norm_capacity, int64_t* norm_doc_offsets, uint8_t* changed, int64_t* counts);

/* ---- UTF-8 validation and repair (td_utf8.hip) --------------------------------------------------------------------------------------------
 * The reference encodes `str`, which is always well-formed UTF-8; the bulk entry points take raw bytes, and what the encoder does with
 * ill-formed bytes is its own (td_common.h).  Text + doc_offsets[n_docs + 1] (int64: from 0, non-decreasing, ending at or below n_bytes)
 * -> flags[d] (uint8: 0 = document d is well-formed), first_bad[d], n_bad[d], and the repaired text + out_doc_offsets[n_docs + 1], which
 * every td_encode_* entry point takes as it stands.  Per document this is exactly CPython's
 * bytes.decode("utf-8", "replace" | "ignore").encode("utf-8").  Host and device compile the same statement of the rule (td_utf8_args.h).
 *   DOCUMENTS  are independent: nothing reaches across a document boundary.  Inside document d, walk from its first byte; at position p:
 *   WELL-FORMED  A well-formed sequence (Unicode Table 3-7: no overlong form, no surrogate, nothing above U+10FFFF) that starts at p and
 *              ends inside the document is one unit.  It is copied.
 *   SUBPART    Otherwise the unit is the maximal subpart (Unicode 3.9, "U+FFFD substitution of maximal subparts", the WHATWG decoder):
 *              the lead byte (C2 .. F4) plus as many following bytes as still form a prefix of some well-formed sequence, the second
 *              byte held to the lead's own range (E0: A0 .. BF, ED: 80 .. 9F, F0: 90 .. BF, F4: 80 .. 8F, else 80 .. BF); a byte that can
 *              start nothing (80 .. BF, C0, C1, F5 .. FF) is a subpart of length one.  TD_UTF8_REPLACE writes EF BF BD for the subpart,
 *              TD_UTF8_IGNORE writes nothing.
 *   CONTEXT    Whether p starts a unit is decided by at most three bytes in front of it: a byte that is no continuation byte always
 *              does; a continuation byte is consumed iff the nearest non-continuation byte q in p - 3 .. p - 1, inside the document, is a
 *              lead that needs more than p - q bytes and text[q + 1] is in that lead's second-byte range.
 *   PER DOCUMENT  flags[d] (uint8), first_bad[d] (int64: the offset inside the document of its first ill-formed subpart, or -1),
 *              n_bad[d] (int64: its ill-formed subparts), out_doc_offsets[n_docs + 1].
 *   counts[8]  (int64) {output bytes needed, documents ill-formed, subparts, bytes in subparts, documents that begin with a
 *              continuation byte, documents whose last unit is a subpart led by a lead byte, 0, 0}.  [4] and [5] say that a chunker cuts
 *              characters.  td_utf8_check_device fills flags, first_bad and counts[1] ALONE, the rest of counts is 0; so does
 *              td_encode_batch_utf8 when no document is flagged: {n_bytes, 0, 0, 0, 0, 0, 0, 0}.
 *   SIZES      TD_UTF8_REPLACE needs at most 3 x the input (a text of stray 80s reaches it), TD_UTF8_IGNORE at most 1 x.  An output that
 *              does not fit is TD_E_CAPACITY (position: the bytes needed, also in counts[0]); nothing is written to `out` or the
 *              offsets.  Bytes behind the last document are not read.
 * Argument errors are TD_E_INVALID before any launch: offsets on the host that do not start at 0 or decrease, a NULL stream, a policy
 * other than the two, an output that overlaps the text.  Results are bitwise reproducible (minima, ors and integer sums only).  Out of
 * scope: other encodings, one U+FFFD per byte, a map from repaired bytes back to source bytes, a NUL or control-character policy,
 * dropping documents (td_select_docs with flags does it). */
#define TD_UTF8_REPLACE 0
#define TD_UTF8_IGNORE 1
/* The contract's executable statement, on the host (no handle, no device).  out may be NULL with out_capacity == 0: out_doc_offsets,
 * flags, first_bad, n_bad (each may be NULL) and counts alone.  Argument errors write nothing. */
int td_utf8_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int policy, uint8_t* out, int64_t out_capacity,
                 int64_t* out_doc_offsets, uint8_t* flags, int64_t* first_bad, int64_t* n_bad, int64_t* counts);
/* DEVICE buffers, asynchronously on hip_stream (never the null stream): no synchronisation and no read-back.  d_doc_offsets, d_counts,
 * d_first_bad, d_n_bad and d_out_doc_offsets are 8-byte aligned; d_text needs no alignment.  Offsets that do not start at 0, decrease,
 * are negative or end above n_bytes raise TD_E_INVALID through td_device_status with err_pos = the lowest such document, and then
 * NOTHING is written.  d_first_bad may be NULL.  counts: [1] alone. */
int td_utf8_check_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                         void* d_flags, void* d_first_bad, void* d_counts, void* hip_stream);
/* d_flags, d_first_bad and d_n_bad may be NULL.  TD_E_CAPACITY surfaces through td_device_status; d_counts[0] holds the bytes needed
 * then, d_out and d_out_doc_offsets are not written. */
int td_utf8_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int policy,
                   void* d_out, int64_t out_capacity, void* d_out_doc_offsets, void* d_flags, void* d_first_bad, void* d_n_bad,
                   void* d_counts, void* hip_stream);
/* Host buffers, synchronously; td_utf8_host's arguments behind the handle.  With out, out_doc_offsets and n_bad all NULL the call is
 * the CHECK (one pass at read speed): flags, first_bad and counts[1] alone, the rest of counts 0. */
int td_utf8(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int policy, uint8_t* out,
            int64_t out_capacity, int64_t* out_doc_offsets, uint8_t* flags, int64_t* first_bad, int64_t* n_bad, int64_t* counts);
/* Upload, check, and td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY only) of the ORIGINAL device buffer when no document is
 * flagged; otherwise the text is repaired into the handle's workspace and that is encoded.  out_tok_offsets[n_docs + 1], and everything
 * later computed from byte positions, refer to the REPAIRED text, which comes back on request: fixed_text (may be NULL with
 * fixed_capacity 0), fixed_doc_offsets, flags, first_bad and n_bad (each may be NULL).  counts: as td_utf8 gives them when a document
 * is flagged, the check's otherwise (counts[8] above).  Synchronous. */
int td_encode_batch_utf8(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int policy,
                         int32_t* out_ids, int64_t ids_capacity, int64_t* out_tok_offsets, uint8_t* fixed_text, int64_t fixed_capacity,
                         int64_t* fixed_doc_offsets, uint8_t* flags, int64_t* first_bad, int64_t* n_bad, int64_t* counts);

/* ---- per-document text statistics for quality filtering (td_textstats.hip) ---------------------------------------------------------------
 * The heuristic quality filters of Gopher, C4 and FineWeb are thresholds on sums and maxima over the per-byte character classes the
 * splitter computes.  Text + doc_offsets[n_docs + 1] (int64: from 0, non-decreasing, ending at or below n_bytes) -> stats[n_docs][TD_TS_COLS]
 * (int64, row-major) and totals[TD_TS_COLS].  No thresholds and no keep / drop policy: the caller builds a mask and hands it to
 * td_select_docs.  Host and device compile the same statement of the rule (td_textstats_args.h).
 *   INPUT      Per document d, over text[doc_offsets[d], doc_offsets[d + 1]): the value the splitter's classification (classify_at,
 *              td_common.h) gives each byte INSIDE that document: a 4-bit class plus F_CONT.  Characters never cross a document start;
 *              ill-formed bytes are C_OTHER characters.  The classes are those of the handle's tables (the cl100k / Qwen2 / GPT-2 pattern
 *              kinds read marks as C_OTHER); td_text_stats_host uses the tables as probed, which are the Llama-4 and generic handles'.
 *   TERMS      A CHARACTER is a byte without F_CONT with the F_CONT bytes behind it.  A SPACE is a character in M_S (\s).  A WORD is a
 *              maximal run of non-space characters.  The LINES are the pieces of the document between bytes 0x0A (the LF is no part of
 *              the line); a final empty piece is no line: "a\n\nb\n" has 3 lines, "" has 0.  A line's first / last VISIBLE character
 *              is its first / last non-space character; a blank line has none.
 *   COLUMNS    0 BYTES  1 CHARS  2 UPPER (C_UP)  3 LOWER (C_LW)  4 LETTER_OTHER (C_LB)  5 MARK (C_MK)  6 NUMBER (C_NUM)  7 SPACE
 *              8 NON_ASCII (characters whose first byte is >= 0x80)  9 WORDS  10 WORDS_ALPHA (words with a character in M_L)
 *              11 WORD_MAX_BYTES (0: no word)  12 LINES  13 LINES_BLANK  14 LINE_MAX_BYTES
 *              15 LINES_END_TERMINAL (last visible character one of . ! ? " U+201D U+3002 U+FF01 U+FF1F)
 *              16 LINES_END_ELLIPSIS (last visible character U+2026, or a '.' with ".." directly in front of it inside the line)
 *              17 LINES_START_BULLET (first visible character one of - * U+2022 U+2023 U+25E6)
 *              18 HASHES (bytes '#')  19 ELLIPSES (characters U+2026, plus maximal runs of three or more '.' bytes inside the document,
 *              a run once)  20 CURLY (bytes '{' or '}')
 *   totals     the sum over all documents of every column but 11 and 14, of which it holds the maximum.
 *   groups     TD_TS_LOCAL: columns 0 - 9, 12, 18 - 20 (each decided by a character and at most three bytes on either side of it; the text
 *              is read once).  TD_TS_RUNS: columns 10, 11, 13 - 17 (they need to know how far back the word or the line began: two more
 *              passes).  Columns of a group that was not asked for are 0.  0, or a value with other bits, is TD_E_INVALID.
 * Bytes behind the last document are not read.  Results are bitwise reproducible (integer sums and maxima only).  Out of scope:
 * duplicate-line and duplicate-n-gram fractions, stop-word rules (td_token_counts serves them), built-in thresholds or presets, lengths in
 * characters for the two maxima. */
#define TD_TS_COLS 21
#define TD_TS_LOCAL 1
#define TD_TS_RUNS 2
/* The contract's executable statement, on the host (no handle, no device).  totals may be NULL.  Argument errors (offsets that do not
 * start at 0 or decrease, groups) are TD_E_INVALID and write nothing. */
int td_text_stats_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats, int64_t* totals);
/* DEVICE buffers, asynchronously on hip_stream (never the null stream): no synchronisation and no read-back.  d_doc_offsets, d_stats and
 * d_totals are 8-byte aligned; d_text needs no alignment; d_totals may be NULL.  Offsets that do not start at 0, decrease, are negative or
 * end above n_bytes raise TD_E_INVALID through td_device_status with err_pos = the lowest such document, and then NOTHING is written. */
int td_text_stats_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int groups,
                         void* d_stats, void* d_totals, void* hip_stream);
/* Host buffers, synchronously; td_text_stats_host's arguments behind the handle. */
int td_text_stats(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats,
                  int64_t* totals);
/* td_encode_batch (TD_MODE_ENCODE / TD_MODE_ORDINARY only) and the statistics of the same upload: the text crosses PCIe once.
 * out_tok_offsets[n_docs + 1]; totals may be NULL.  Synchronous. */
int td_encode_batch_text_stats(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int groups,
                               int32_t* out_ids, int64_t ids_capacity, int64_t* out_tok_offsets, int64_t* stats, int64_t* totals);

/* Options. */
#define TD_OPT_LONG_POOL_BYTES 1 /* scratch for pieces longer than 64 bytes (default max(64 MiB, 2 x input)) */
#define TD_OPT_PROFILE 2         /* 1: bracket the kernels of every td_encode_device call with HIP events on the
                                    call's stream (td_profile_read_ex) */
#define TD_OPT_PIPE_CHUNK_BYTES 3 /* td_encode_batch cuts inputs of at least HALF this many bytes (default 64 MiB) into chunks of whole
                                    documents of about this size — a sixth of the input, down to an eighth of the size, when the input
                                    is less than six chunks — and overlaps host copies, PCIe transfers (both directions) and kernels */
#define TD_OPT_SMALL_PATH 5       /* 0: never take the one-launch path for inputs of at most 4 KiB (default 1: on) */
#define TD_OPT_FUSED 6            /* 0: pre-tokenizer and lookup as two kernels, two passes over the text (default 1: one fused pass;
                                    TD_FUSED=0 in the environment at td_create time also turns it off).  Same results either way. */
#define TD_OPT_GRAPH 7            /* 1: replay a repeated td_encode_device call as a hipGraph (default 0: off; TD_GRAPH=1 in the environment
                                    at td_create time also turns it on): the second identical call in a row captures the step's launches on
                                    a PRIVATE non-blocking stream of the handle (the caller's stream is never put into capture), the
                                    following ones are one hipGraphLaunch on the caller's stream.  A capture that fails is ended and the
                                    step is launched kernel by kernel; same results either way. */
#define TD_OPT_DEVICE_SPECIALS 8  /* 0: td_encode_batch_with_special* always search for the allowed specials on host threads (default 1:
                                    batches of a MiB and more search on the device, td_special.hip; same results) */
#define TD_OPT_DIRECT 9            /* 0 (default): every tile's ids are staged and packed (rounds 1-3).  1 (measured slower): the fused tile loop
                                    writes a tile's ids straight to the output when the tile's base is known in time (decoupled look-back
                                    over per-tile id counts; tiles that are not — and everything behind a tile whose count cannot be settled
                                    inside the loop — are staged as before).  Same results either way; TD_DIRECT=1 in the environment at
                                    td_create time also turns it on. */
#define TD_OPT_PACK_SPLIT 10       /* 1 (default): the ids are placed by a pair of kernels — td_pack_plain, a wavefront per tile that has no long
                                    piece and at most a few merged ones (nearly a copy: 5 TB/s), and td_pack_rest for the others; 0: one
                                    kernel for all tiles (td_pack_tokens, rounds 2-4).  Same results either way; TD_PACK_SPLIT=0 in the
                                    environment at td_create time also turns it off. */
#define TD_OPT_DEDUPE 11           /* 1 (default): a piece that is not a token is merged ONCE per call however often its bytes occur in it — the
                                    pieces of the tiles with many missed pieces are looked up in a table of the call's distinct ones (bytes
                                    compared, not hashes) and the repeats copy the ids; 0: every piece is merged (rounds 1-4).  Same results
                                    either way (bpe_merge reads nothing but the piece, tiktoken.cpp:298-368); TD_DEDUPE=0 in the environment at
                                    td_create time also turns it off. */
#define TD_OPT_OVERLAP 12          /* 1 (default): once the handle has seen long pieces (>= 2048 in the last call whose counters were read:
                                    td_device_status and every host-buffer entry point read them), the kernels of the pieces above 64 bytes run on
                                    a second stream of the handle beside the kernels of the shorter ones (fork behind the lookups, join in front of
                                    the scan; parallel branches when the step is captured into a graph); 0: always one kernel after the other.
                                    Same results either way; TD_OVERLAP=0 in the environment at td_create time also turns it off. */
#define TD_OPT_GIANT_COOP_MIN 13   /* bytes (default 16384, at least 1024): a single piece above this length is merged by ALL workgroups of
                                    td_giant_pieces together (grid barriers between the sweeps; a megabyte of random letters: 0.55 s on one
                                    workgroup); shorter pieces above 1 KiB get a workgroup each as before.  Same results either way;
                                    TD_GP_COOP_MIN in the environment at td_create time sets it too. */
#define TD_OPT_SPARSE 14           /* The launch sequence of a step.  -1 (default): chosen by the counters of the last call that were read
                                    (td_device_status and every host-buffer entry point read them): text that leaves the kernels for far
                                    pieces, deferred and flagged tiles and long pieces (nearly) idle — plain prose — takes the SPARSE
                                    sequence, six launches (td_prepare_mark, td_split_tiles, td_tail, td_giant_scan, td_pack_plain,
                                    td_pack_rest); other text, and a handle whose counters nobody has read yet, the DENSE one, where those
                                    kernels are launches of their own at their own occupancies.  1: always sparse, 0: always dense.  Same
                                    results either way — td_tail walks every phase the dense sequence has kernels for; TD_SPARSE in the
                                    environment at td_create time sets it too. */
#define TD_OPT_PIPE_THREADS 4     /* host threads that fill / drain the pinned bounce buffers of that pipeline (default 16) */
#define TD_OPT_COUNTS_SEATS 15     /* seats of the on-chip table of td_token_counts*: a power of two from 2 to the production size
                                    (4096), or 0 (default) for that.  Same results whatever it is; tests force the conflict path with 2. */
#define TD_OPT_COUNTS_FLUSH_TILES 16 /* tiles (4096 ids) a workgroup of td_token_counts* counts between two flushes of that table: 1 to the
                                    production interval (64), or 0 (default) for that.  Same results whatever it is; tests shrink it, a call
                                    needs more than 268 M ids to reach the production interval. */
#define TD_OPT_NGRAM_TAG_BITS 17   /* the hash bits a lookup of td_ngram_matches* compares before it compares ids: 1 to 31, or 0 (default) for the
                                    production width, all 32.  Same results whatever it is; tests set 1 to 4 so that lookups whose hash
                                    bits agree and whose ids differ are walked. */
#define TD_OPT_WS_FILL 18          /* debugging: -1 (default) off; 0..255: every device buffer the handle allocates from now on is filled
                                    with this byte over its whole capacity when it is allocated, and every buffer of the step workspace
                                    (all but the control block's first 256 bytes) again in front of every step of td_encode_device and of
                                    whatever ends in one, on the call's stream.  A kernel that reads a workspace word nobody wrote in this
                                    call then reads this byte, not what the allocator or the last call left: results must not depend on
                                    it.  TD_INFO_WS_FILLED_BYTES counts what was filled.  TD_WS_FILL in the environment at td_create time
                                    sets it too (td_create's own allocations included); td_clone hands it on.  Off: one branch per
                                    allocation and per step. */
int td_set_option(td_tokenizer* t, int what, int64_t value);

/* Sums (ms) of the pre-tokenizer kernel and token kernel (probe + merge) durations and the number of calls recorded
 * since the last read (TD_OPT_PROFILE); synchronises the recorded events. */
int td_profile_read(td_tokenizer* t, double* split_ms_sum, double* encode_ms_sum, int64_t* launches);
/* The same per kernel segment: ms_sums[i] = summed duration of segment i (td_profile_segment_name(i); "" past the last
 * one) over the calls recorded since the last read. */
int td_profile_read_ex(td_tokenizer* t, double* ms_sums, int n_segments, int64_t* launches);
const char* td_profile_segment_name(int i);

/* Special-token table access: replaces CoreBPE::special_tokens() (tiktoken.cpp:258-265). */
int64_t td_special_count(const td_tokenizer* t);
int td_special_get(const td_tokenizer* t, int64_t i, const char** str, int64_t* len, int32_t* id);

/* Batch decode (replaces the thread pool of Tokenizer.decode_batch, tokendagger/wrapper.py:237-256): the ids of all
 * documents concatenated + tok_offsets[n_docs+1] -> the bytes of all documents concatenated + out_offsets[n_docs+1],
 * one device pass.  *n_bytes = total bytes (also on TD_E_CAPACITY). */
int td_decode_batch(td_tokenizer* t, const int32_t* tokens, const int64_t* tok_offsets, int64_t n_docs, uint8_t* out,
                    int64_t out_capacity, int64_t* out_offsets, int64_t* n_bytes);

/* Device-resident decode: d_tokens int32[n_tokens] -> d_out bytes (capacity out_capacity), total byte count to
 * *d_n_bytes (device int64, may be NULL).  Asynchronous on hip_stream; an id outside the vocabulary (TD_E_BAD_TOKEN,
 * position = its index) or a too small d_out (TD_E_CAPACITY, position = bytes needed) surface through
 * td_device_status.  Same semantics as td_decode_bytes / CoreBPE::decode_bytes (tiktoken.cpp:236-255). */
int td_decode_device(td_tokenizer* t, const void* d_tokens, int64_t n_tokens, void* d_out, int64_t out_capacity,
                     void* d_n_bytes, void* hip_stream);

/* ---- decode rows: segments, a skip set, a stop set, negative ids (td_decode_rows.hip) ---------------------------------------------
 * ids[n_tokens] (int32) in n_segs segments -> the segments' bytes concatenated in `out`, out_offsets[n_segs + 1] (int64, the first
 * 0), seg_ids[n_segs] (int64, may be NULL: the ids each segment consumed) and info[4] (int64: bytes, ids emitted, ids skipped,
 * segments stopped).  What Hugging Face's batch_decode(skip_special_tokens=True) does to a generated batch, what turns PAD / WINDOWS /
 * CONCAT / BESTFIT rows back into text, and what prints the text a label stream trains on.
 *   Segments, offsets form (row_stride == 0): tok_offsets[n_segs + 1] (int64), non-decreasing, 0 <= tok_offsets[0],
 *     tok_offsets[n_segs] <= n_tokens; segment d is ids[tok_offsets[d], tok_offsets[d + 1]).  seg_len is ignored.  Encoded
 *     documents, cu_seqlens.
 *   Segments, rows form (row_stride >= 1): n_segs * row_stride <= n_tokens; segment r is ids[r * row_stride, r * row_stride + len_r)
 *     with len_r = seg_len ? seg_len[r] : row_stride (int32) and 0 <= len_r <= row_stride.  tok_offsets is ignored.  Generation
 *     output, PAD / WINDOWS rows with their lengths.
 *   The rule.  A segment is walked left to right and starts open:
 *     1. once it has stopped no further id of it is looked at: what lies there emits nothing, raises nothing, counts in nothing;
 *     2. id < 0: skipped under TD_DECODE_SKIP_NEGATIVE, otherwise TD_E_BAD_TOKEN at its index;
 *     3. an id of the stop set stops the segment; its bytes are emitted only under TD_DECODE_KEEP_STOP and only if it is not also
 *        skipped (by rule 4).  seg_ids[d] = the ids consumed, the stop id included; the segment's length if it never stopped;
 *     4. an id of the skip set, and under TD_DECODE_SKIP_SPECIAL every special id of the handle's vocabulary, emits nothing;
 *     5. any other id emits its token's bytes (a special token its literal); an id that is no token is TD_E_BAD_TOKEN.  A kept stop
 *        id that is no token is one too.  The lowest index wins.
 *     info[1] counts the consumed ids that emitted bytes, info[2] those that emitted none by rules 2 - 4; info[1] + info[2] is
 *     the sum of seg_ids.
 *   Listed ids must be >= 0 (TD_E_INVALID), may repeat, and may lie above the vocabulary (models pad with n_vocab); at most 65535
 *     distinct listed ids may lie above it.
 *   Capacity.  More bytes than out_capacity: TD_E_CAPACITY, position = the bytes needed; out_offsets, seg_ids and info are complete
 *     and right, no byte is written.  A NULL out with capacity 0 is the sizing call.
 *   Bounds.  Whatever the ids, offsets and lengths hold: nothing outside ids[0, n_tokens), tok_offsets[0 .. n_segs] and
 *     seg_len[0, n_segs) is read, nothing outside the outputs is written.  Outputs of a call that raised TD_E_INVALID are unspecified. */
#define TD_DECODE_KEEP_STOP 1
#define TD_DECODE_SKIP_NEGATIVE 2
#define TD_DECODE_SKIP_SPECIAL 4
typedef struct td_decode_spec {
    int64_t row_stride;      /* 0: segments come from tok_offsets; >= 1: segment r = ids[r*row_stride, r*row_stride + len_r) */
    const int32_t* skip_ids; /* host pointers, read before the call returns; any order, duplicates allowed */
    int64_t n_skip;
    const int32_t* stop_ids;
    int64_t n_stop;
    int64_t flags;           /* TD_DECODE_KEEP_STOP | TD_DECODE_SKIP_NEGATIVE | TD_DECODE_SKIP_SPECIAL */
} td_decode_spec;

/* The argument checks, on the host (no handle, no device): TD_OK or TD_E_INVALID with *bad_pos (may be NULL) = the offending index:
 * a segment (decreasing tok_offsets[d + 1] < tok_offsets[d]: d; tok_offsets[0] < 0: 0; tok_offsets[n_segs] > n_tokens: n_segs;
 * a seg_len[r] outside [0, row_stride]: r), the index of a negative listed id in skip_ids followed by stop_ids (i, or n_skip + i),
 * or -1 for everything else (a NULL spec, unknown flags, negative sizes, a NULL list with entries, a NULL tok_offsets in the
 * offsets form, n_segs * row_stride > n_tokens). */
int td_decode_rows_check(const td_decode_spec* spec, int64_t n_tokens, const int64_t* tok_offsets, const int32_t* seg_len,
                         int64_t n_segs, int64_t* bad_pos);
/* Host buffers, synchronously.  The arguments are checked with td_decode_rows_check before anything is launched.  *n_bytes (may be
 * NULL) = the bytes needed, also on TD_E_CAPACITY, where out_offsets, seg_ids and info are filled as well. */
int td_decode_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, const int32_t* seg_len,
                   int64_t n_segs, const td_decode_spec* spec, uint8_t* out, int64_t out_capacity, int64_t* out_offsets,
                   int64_t* seg_ids, int64_t* info, int64_t* n_bytes);
/* DEVICE buffers, asynchronously on hip_stream: no synchronisation and no read-back; errors surface through td_device_status
 * (TD_E_BAD_TOKEN: the id's index; TD_E_CAPACITY: the bytes needed; TD_E_INVALID: the segment whose offset decreases or whose
 * length is outside [0, row_stride]).  d_out_offsets, d_seg_ids (may be NULL) and d_info are 8-byte aligned device memory.  The
 * spec's lists are host memory and are read before the call returns. */
int td_decode_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, const void* d_seg_len,
                          int64_t n_segs, const td_decode_spec* spec, void* d_out, int64_t out_capacity, void* d_out_offsets,
                          void* d_seg_ids, void* d_info, void* hip_stream);

/* Vocabulary accessors (host tables, no launch): the bytes of one token id (tiktoken decode_single_token_bytes;
 * TD_E_BAD_TOKEN if the id is not in the vocabulary) and the id of one whole token (tiktoken encode_single_token:
 * regular tokens first, then special tokens; TD_E_UNKNOWN_BYTE if the bytes are not a token). */
int td_token_bytes(const td_tokenizer* t, int32_t id, const uint8_t** bytes, int64_t* len);
int td_single_token(const td_tokenizer* t, const uint8_t* bytes, int64_t len, int32_t* id);

/* ---- vocabulary files (host only; no GPU needed) ------------------------------------------------------------
 * Replaces the reference's loaders, which live in its demo and in Python: LoadBPEFile / LoadTokenizer
 * (src/main.cpp:70-137), load_bpe_vocab / load_special_tokens / load_mistral_config (tests/throughput_test.py:
 * 106-180) and Tokenizer._load_vocab_file / _load_special_tokens_file (tokendagger/wrapper.py:116-134).
 * A td_vocab accumulates regular tokens, special tokens and (tekken only) the split pattern; every loader appends.
 * All return TD_OK, TD_E_INVALID (bad argument) or TD_E_VOCAB (unreadable / malformed file: td_vocab_error). */
typedef struct td_vocab td_vocab;
int td_vocab_create(td_vocab** out);
void td_vocab_destroy(td_vocab* v);
const char* td_vocab_error(const td_vocab* v);
/* tiktoken ".model": lines of "<base64 token bytes> <rank>" */
int td_vocab_load_tiktoken(td_vocab* v, const char* path);
/* Hugging Face tokenizer_config.json: added_tokens_decoder {"<id>": {"content": "..."}} -> special tokens;
 * also_mergeable != 0 additionally enters them as regular tokens, as the reference's tests do
 * (tests/throughput_test.py:211-213). */
int td_vocab_load_hf_special(td_vocab* v, const char* path, int also_mergeable);
/* Mistral tekken.json: config.pattern + the first default_vocab_size - default_num_special_tokens entries of
 * "vocab", id = index + default_num_special_tokens */
int td_vocab_load_tekken(td_vocab* v, const char* path);
/* the reference wrapper's JSON files; either path may be NULL */
int td_vocab_load_json(td_vocab* v, const char* vocab_json_path, const char* special_json_path);
int td_vocab_set_pattern(td_vocab* v, const char* pat_str);
const char* td_vocab_pattern(const td_vocab* v); /* "" if none was set / loaded */
/* flat views (valid until the next load / destroy): which = 0 regular, 1 special */
int td_vocab_arrays(const td_vocab* v, int which, const uint8_t** bytes, const int64_t** offsets, const int32_t** ranks,
                    int64_t* n);
/* td_create over a loaded vocabulary (pattern = td_vocab_pattern) */
int td_create_from_vocab(const td_vocab* v, int device, td_tokenizer** out);

/*
 * Multi-GPU epilogue (one process per GPU, documents sharded across ranks).  The reference parallelises over
 * independent texts on a thread pool (tokendagger/wrapper.py:231-235) and needs no exchange; across GPUs the only one is
 * the gather of every rank's {tokens, documents} -> global token / document bases, and optionally of the ids to one rank.
 * RCCL (over xGMI on an MI355X node) is opened at run time; the tokenizer library links against HIP only.
 *   td_comm_unique_id      rank 0 makes the id (ncclGetUniqueId); the caller carries its 128 bytes to the other ranks
 *   td_comm_create         ncclCommInitRank on `device` (-1: the current device); collective over all ranks
 *   td_comm_gather_counts  ncclAllGather of d_counts[2] = {tokens, documents} (device memory: e.g. elements n_docs and
 *                          n_docs + 1 of the offsets buffer td_encode_device wrote, with the document count stored behind the
 *                          total) into d_table[2 * world] on every rank; asynchronous on `stream`
 *   td_comm_bases          host: exclusive prefix sums of a gathered table -> this rank's token / document base and the totals
 *   td_comm_gather_tokens  grouped ncclSend / ncclRecv: every rank's ids (table[2 r] of them) end up contiguous, in rank order,
 *                          in d_root_tokens on `root`; `table` is the gathered table on the HOST; asynchronous on `stream`.
 *                          A root buffer that is too small fails on the ROOT only (TD_E_CAPACITY), after the root has taken
 *                          the other ranks' ids into a scratch buffer: no rank is left with a pending send.
 */
#define TD_COMM_ID_BYTES 128
typedef struct td_comm td_comm;
int td_comm_unique_id(uint8_t id[TD_COMM_ID_BYTES]);
int td_comm_create(const uint8_t id[TD_COMM_ID_BYTES], int world, int rank, int device, td_comm** out);
void td_comm_destroy(td_comm* c);
int td_comm_gather_counts(td_comm* c, const int64_t* d_counts, int64_t* d_table, void* stream);
int td_comm_bases(const int64_t* table, int world, int rank, int64_t* token_base, int64_t* doc_base, int64_t* token_total,
                  int64_t* doc_total);
int td_comm_gather_tokens(td_comm* c, const int32_t* d_tokens, const int64_t* table, int root, int32_t* d_root_tokens,
                          int64_t root_capacity, void* stream);
const char* td_comm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TOKENDAGGER_HIP_H */
