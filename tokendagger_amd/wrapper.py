"""tiktoken-compatible Python surface over the MI355X tokenizer core.

Mirrors the public interface of the reference's ``tokendagger`` package (class / function names,
keyword arguments, defaults, exception types: /root/reference/tokendagger/wrapper.py:28-395) so that
``import tokendagger as tiktoken`` keeps working, but every encode/decode goes to the HIP library
through ``_tokendagger_core`` — there is no CPU tokenization in this package.  Batch methods hand the
whole batch to the GPU in one call instead of fanning single calls out to a thread pool
(reference: wrapper.py:212-235); ``num_threads`` is accepted for compatibility and ignored.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import AbstractSet, Collection, Literal, NamedTuple, Sequence

import numpy as np

from . import capi as _capi

_capi.load_library()  # (first: it makes the HIP runtime of this process the one torch bundles, when torch is installed)
from . import _tokendagger_core as _core  # noqa: E402

MODE_ENCODE, MODE_ORDINARY = 0, 1
_UNITS = {"bytes": 0, "chars": 1}  # TD_UNIT_BYTES, TD_UNIT_CHARS
_LAYOUTS = {"concat": 0, "pad": 1}  # TD_ROWS_CONCAT, TD_ROWS_PAD


class Rows(NamedTuple):
    """Training rows (Tokenizer.encode_batch_to_rows / ids_to_rows; the contract: include/tokendagger_hip.h, td_make_rows)."""
    ids: np.ndarray                 # int32 [rows, seq_len]
    positions: np.ndarray | None    # int32 [rows, seq_len]: the index inside the segment (concat) / row (pad); pad slots 0
    cu_seqlens: np.ndarray | None   # int32 [n_seg + 1]: "concat" segment boundaries 0 .. real slots
    lengths: np.ndarray | None      # int32 [n_docs]: "pad" real slots of every row
    counts: np.ndarray              # int64 [4]: rows, real slots, segments, truncated documents


class PackedRows(NamedTuple):
    """Whole documents packed into rows by best-fit decreasing (Tokenizer.ids_to_packed_rows / encode_batch_to_packed_rows; the
    contract: include/tokendagger_hip.h, TD_ROWS_BESTFIT)."""
    ids: np.ndarray                 # int32 [rows, seq_len]
    positions: np.ndarray | None    # int32 [rows, seq_len]: the index inside the segment; pad slots 0
    cu_seqlens: np.ndarray | None   # int32 [segments + 1]: segment boundaries over the flattened rows, pad tails included
    lengths: np.ndarray             # int32 [rows]: real slots of every row
    docs: np.ndarray | None         # int64 [segments]: the document of every segment, -1 for a pad tail
    counts: np.ndarray              # int64 [4]: rows, real slots, segments, documents cut


class WindowRows(NamedTuple):
    """One document per row, a longer document continued in overlapping rows of its own (Tokenizer.ids_to_window_rows /
    encode_batch_to_window_rows; the contract: include/tokendagger_hip.h, TD_ROWS_WINDOWS)."""
    ids: np.ndarray                 # int32 [rows, seq_len]
    positions: np.ndarray | None    # int32 [rows, seq_len]: the index inside the row; pad slots 0
    lengths: np.ndarray             # int32 [rows]: real slots of every row
    docs: np.ndarray                # int64 [rows]: the row's document
    starts: np.ndarray              # int64 [rows]: the index of the row's first body id inside its document
    counts: np.ndarray              # int64 [4]: rows, real slots, documents with more than one window, the most windows of one


class LabeledRows(NamedTuple):
    """Trainer-ready rows: the id rows of a layout and the label rows placed beside them in the same pass
    (Tokenizer.ids_to_labeled_rows / encode_batch_to_labeled_rows; the contract: include/tokendagger_hip.h, td_rows_labels)."""
    rows: "Rows | PackedRows | WindowRows"  # the layout's own rows
    labels: np.ndarray                      # int32 [rows, seq_len]


class Labels(NamedTuple):
    """Loss labels for marked id spans (Tokenizer.ids_to_labels / encode_batch_to_labels; the contract:
    include/tokendagger_hip.h, td_labels_spec) or for byte ranges (ids_to_range_labels / encode_batch_to_range_labels;
    td_range_spec: counts = trained ids, partially marked ids, marked bytes, 0)."""
    ids: np.ndarray                     # int32 [total]
    tok_offsets: np.ndarray             # int64 [n_docs + 1]
    labels: np.ndarray                  # int32 [total]: the id where the loss applies, ignore_index elsewhere
    mask: np.ndarray | None             # uint8 [total]: 1 where the loss applies
    trained_offsets: np.ndarray | None  # int64 [n_docs + 1]: trained ids in front of every document, the total last
    counts: np.ndarray                  # int64 [4]: trained ids, spans, unterminated documents, 0


class TokenCounts(NamedTuple):
    """Histograms of ids (Tokenizer.ids_to_counts; the contract: include/tokendagger_hip.h, td_counts_spec)."""
    counts: np.ndarray  # int64 [n_groups, n_bins], or [n_bins] without groups
    counted: int        # positions added to counts
    negative: int       # positions with a negative value (the ignore_index of a label stream)
    too_large: int      # positions with a value >= n_bins


class EncodedTokenCounts(NamedTuple):
    """Tokenizer.encode_batch_to_counts: TokenCounts and the ids the encode made."""
    counts: np.ndarray
    counted: int
    negative: int
    too_large: int
    n_tokens: int


class NgramMatches(NamedTuple):
    """Listed id sequences found in documents (Tokenizer.ids_to_ngram_matches / encode_batch_to_ngram_matches; the contract:
    include/tokendagger_hip.h, td_ngram_spec)."""
    cover: np.ndarray | None           # uint8 [total]: 1 where the id lies inside an occurrence
    labels: np.ndarray | None          # int32 [total]: the labels given, ignore_index where covered
    doc_stats: np.ndarray | None       # int64 [n_docs, 2]: occurrences starting in the document, its covered ids
    pattern_counts: np.ndarray | None  # int64 [n_pats]: occurrences of every pattern (a repeated one under its lowest index)
    counts: np.ndarray                 # int64 [4]: occurrences, covered ids, documents with an occurrence, 0


class MinHashes(NamedTuple):
    """MinHash signatures and LSH band keys per document (Tokenizer.ids_to_minhash / encode_batch_to_minhash; the contract:
    include/tokendagger_hip.h, td_minhash_spec)."""
    signatures: np.ndarray        # uint32 [n_docs, num_perm]; all 0xFFFFFFFF for a document with no id
    band_keys: np.ndarray | None  # uint64 [n_docs, bands]: equal keys in the same band mean "candidate pair"
    counts: np.ndarray            # int64 [4]: shingles hashed, documents with no id, documents of 1 .. ngram - 1 ids, 0

    def similarity(self, i: int, j: int) -> float:
        """The fraction of equal signature entries of documents i and j: an unbiased estimate of the Jaccard similarity of their
        shingle sets, with standard deviation sqrt(J (1 - J) / num_perm)."""
        return float(np.mean(self.signatures[i] == self.signatures[j]))


class NormalizedText(NamedTuple):
    """Tokenizer.normalize_batch (the contract: include/tokendagger_hip.h, td_nfc*): text + offsets go to every bulk method as they stand."""
    text: np.ndarray     # uint8: the documents' NFC, concatenated
    offsets: np.ndarray  # int64 [n_docs + 1]
    flags: np.ndarray | None  # uint8 [n_docs]: 0 = the document was proven to be NFC already, 1 = not proven
    changed: np.ndarray  # uint8 [n_docs]: 1 = the document's bytes differ
    counts: np.ndarray   # int64 [8]: output bytes, documents not proven, documents changed, segments rewritten, code points in them,
                         # opaque bytes, the longest segment in code points, 0


class ValidatedText(NamedTuple):
    """Tokenizer.validate_batch (the contract: include/tokendagger_hip.h, td_utf8*)."""
    flags: np.ndarray      # uint8 [n_docs]: 0 = the document is well-formed UTF-8
    first_bad: np.ndarray  # int64 [n_docs]: the offset inside the document of its first ill-formed subpart, or -1
    counts: np.ndarray     # int64 [8]: counts[1] = documents ill-formed; the rest is 0 (the check counts nothing else)


class RepairedText(NamedTuple):
    """Tokenizer.repair_batch: text + offsets go to every bulk method as they stand."""
    text: np.ndarray       # uint8: the documents' bytes.decode("utf-8", errors).encode("utf-8"), concatenated
    offsets: np.ndarray    # int64 [n_docs + 1]
    flags: np.ndarray      # uint8 [n_docs]: 0 = the document was well-formed
    first_bad: np.ndarray  # int64 [n_docs]
    n_bad: np.ndarray      # int64 [n_docs]: the document's ill-formed subparts
    counts: np.ndarray     # int64 [8]: output bytes, documents ill-formed, subparts, bytes in subparts, documents that begin with a
                           # continuation byte, documents whose last unit is a subpart led by a lead byte, 0, 0


class TextStats:
    """Tokenizer.text_stats (the contract: include/tokendagger_hip.h, td_text_stats*): the statistics the heuristic quality filters are
    built from.  No thresholds here: build a mask from the columns and the ratios and hand the kept documents to select_docs."""

    def __init__(self, stats: np.ndarray, totals: np.ndarray):
        self.stats = stats    # int64 [n_docs, 21]
        self.totals = totals  # int64 [21]: the columns' sums, the maximum of word_max_bytes and line_max_bytes

    def __getattr__(self, name):  # the named column views: .words, .lines_end_terminal, ... (capi.TS_COLUMNS)
        if name in _capi.TS_COLUMNS:
            return self.stats[:, _capi.TS_COLUMNS.index(name)]
        raise AttributeError(name)

    def _ratio(self, num, den) -> np.ndarray:
        """num / den per document as float64, 0.0 where den is 0"""
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        return np.divide(num, den, out=np.zeros_like(num), where=den != 0)

    @property
    def mean_word_bytes(self) -> np.ndarray:
        """(bytes - space characters) / words: the words' mean length in bytes.  Exact where every space character is one byte; a space
        of two or three bytes (U+00A0, U+3000, ...) leaves its other bytes with the words."""
        return self._ratio(self.bytes - self.space, self.words)

    @property
    def alpha_word_fraction(self) -> np.ndarray:
        return self._ratio(self.words_alpha, self.words)

    @property
    def terminal_line_fraction(self) -> np.ndarray:
        return self._ratio(self.lines_end_terminal, self.lines)

    @property
    def ellipsis_line_fraction(self) -> np.ndarray:
        return self._ratio(self.lines_end_ellipsis, self.lines)

    @property
    def bullet_line_fraction(self) -> np.ndarray:
        return self._ratio(self.lines_start_bullet, self.lines)

    @property
    def symbol_word_ratio(self) -> np.ndarray:
        """'#' bytes and ellipses over words"""
        return self._ratio(self.hashes + self.ellipses, self.words)

    @property
    def upper_letter_fraction(self) -> np.ndarray:
        return self._ratio(self.upper, self.upper + self.lower + self.letter_other)


_TS_GROUPS = {"all": _capi.TD_TS_ALL, "local": _capi.TD_TS_LOCAL, "runs": _capi.TD_TS_RUNS}


def _ts_groups(groups):
    if groups not in _TS_GROUPS:
        raise ValueError(f"groups must be 'all', 'local' or 'runs', not {groups!r}")
    return _TS_GROUPS[groups]


_UTF8_ERRORS = {"replace": _capi.TD_UTF8_REPLACE, "ignore": _capi.TD_UTF8_IGNORE}


def _utf8_policy(errors):
    if errors not in _UTF8_ERRORS:
        raise ValueError(f"errors must be 'replace' or 'ignore', not {errors!r}")
    return _UTF8_ERRORS[errors]


_NORMALIZERS = (None, "NFC")


def _check_normalizer(normalizer):
    if normalizer not in _NORMALIZERS:
        raise ValueError(f"normalizer must be None or 'NFC', not {normalizer!r}")
    return normalizer


class DecodedRows(NamedTuple):
    """Tokenizer.decode_rows_to_numpy (the contract: include/tokendagger_hip.h, td_decode_spec)."""
    data: np.ndarray     # uint8: the segments' bytes, concatenated
    offsets: np.ndarray  # int64 [n_segs + 1]: segment d is data[offsets[d]:offsets[d + 1]]
    seg_ids: np.ndarray  # int64 [n_segs]: the ids each segment consumed, its stop id included
    n_emitted: int       # ids that emitted bytes
    n_skipped: int       # ids consumed that emitted none
    n_stopped: int       # segments a stop id ended


class JoinedFields(NamedTuple):
    """Examples built from several encoded fields (Tokenizer.join_fields / encode_fields; the contract: include/tokendagger_hip.h,
    td_join_spec).  ids + offsets (+ labels) feed ids_to_labeled_rows, select_docs and the rest unchanged."""
    ids: np.ndarray               # int32 [T]: per kept example, before_0 body_0 ... before_{K-1} body_{K-1} tail
    labels: np.ndarray | None     # int32 [T]: the id where its part is trained, ignore_index elsewhere
    types: np.ndarray | None      # int32 [T]: the field's type value, the tail's on the tail
    offsets: np.ndarray           # int64 [E + 1]: example k is ids[offsets[k]:offsets[k + 1]]
    examples: np.ndarray          # int64 [E]: the input example that output example k is
    field_len: np.ndarray         # int32 [E, K]: the ids kept of every field
    counts: np.ndarray            # int64 [4]: kept examples E, kept slots T, examples dropped, examples truncated


class TokenDaggerError(Exception):
    """Base exception for TokenDagger errors (reference: wrapper.py:23-25)."""


def _vocab_items(vocab) -> list:
    """Accepts the reference's list-of-dicts form ({'rank','token_bytes','token_string'}) or a tiktoken
    ``mergeable_ranks`` dict {bytes: rank}."""
    items = []
    if isinstance(vocab, dict):
        for token_bytes, rank in vocab.items():
            it = _core.VocabItem()
            it.rank = int(rank)
            it.token_bytes = list(token_bytes)
            items.append(it)
        return items
    for entry in vocab:
        it = _core.VocabItem()
        it.rank = int(entry["rank"])
        it.token_bytes = list(entry["token_bytes"])
        it.token_string = entry.get("token_string", "")
        items.append(it)
    return items


class Tokenizer:
    """High-level tokenizer with the tiktoken ``Encoding`` methods (reference: wrapper.py:28-326)."""

    def __init__(
        self,
        name: str,
        *,
        pattern: str | None = None,
        pat_str: str | None = None,
        vocab: list[dict] | None = None,
        mergeable_ranks: dict[bytes, int] | None = None,
        special_tokens: dict[str, int] | None = None,
        vocab_file: str | Path | None = None,
        special_tokens_file: str | Path | None = None,
        device: int = -1,
        normalizer: str | None = None,
    ):
        self.name = name
        self.normalizer = _check_normalizer(normalizer)
        self.pattern = pat_str if pat_str is not None else pattern
        if mergeable_ranks is not None:
            vocab = mergeable_ranks
        if vocab_file:
            vocab = self._read_json(vocab_file, "Vocabulary")
        elif vocab is None:
            raise ValueError("Either 'vocab', 'mergeable_ranks', or 'vocab_file' must be provided")
        if special_tokens_file:
            special_tokens = self._read_json(special_tokens_file, "Special tokens")
        elif special_tokens is None:
            special_tokens = {}
        self._special_tokens = dict(special_tokens)
        ranks = list(vocab.values()) if isinstance(vocab, dict) else [e["rank"] for e in vocab]
        self.max_token_value = max(max(ranks), max(self._special_tokens.values()) if self._special_tokens else 0)
        specials = []
        for text, rank in self._special_tokens.items():
            it = _core.VocabItem()
            it.rank = int(rank)
            it.token_bytes = list(text.encode("utf-8"))
            it.token_string = text
            specials.append(it)
        try:
            self._core_bpe = _core.CoreBPE(self.pattern, _vocab_items(vocab), specials, device)
        except Exception as e:
            raise TokenDaggerError(f"Failed to initialize CoreBPE: {e}")

    @classmethod
    def from_files(cls, name: str, *, pat_str: str | None = None, tiktoken_model: str | Path | None = None,
                   hf_config: str | Path | None = None, specials_mergeable: bool = False,
                   tekken: str | Path | None = None, vocab_file: str | Path | None = None,
                   special_tokens_file: str | Path | None = None, device: int = -1, normalizer: str | None = None) -> "Tokenizer":
        """Build a tokenizer straight from vocabulary files with the C++ loaders (no per-token Python objects):
        a tiktoken ``.model`` (+ optional Hugging Face ``tokenizer_config.json`` for the special tokens, which
        ``specials_mergeable`` also enters as ordinary tokens the way the reference's benchmarks do), a Mistral
        ``tekken.json`` (carries its own pattern), or the reference wrapper's JSON files."""
        for p in (tiktoken_model, hf_config, tekken, vocab_file, special_tokens_file):
            if p is not None and not Path(p).exists():
                raise FileNotFoundError(f"Vocabulary file not found: {p}")
        s = lambda p: "" if p is None else str(p)
        self = cls.__new__(cls)
        self.name = name
        self.normalizer = _check_normalizer(normalizer)
        try:
            self._core_bpe = _core.CoreBPE.from_files(pat_str or "", s(tiktoken_model), s(hf_config), specials_mergeable,
                                                      s(tekken), s(vocab_file), s(special_tokens_file), device)
        except Exception as e:
            raise TokenDaggerError(f"Failed to initialize CoreBPE: {e}")
        self.pattern = self._core_bpe.pattern()
        self._special_tokens = dict(self._core_bpe.special_map())
        self.max_token_value = int(self._core_bpe.info(3))
        return self

    @staticmethod
    def _read_json(path, what):
        p = Path(path)
        if not p.exists():
            raise FileNotFoundError(f"{what} file not found: {p}")
        with open(p, "r", encoding="utf-8") as f:
            return json.load(f)

    def __repr__(self) -> str:
        return f"<TokenDagger {self.name!r}>"

    # ------------------------------------------------------------------ encoding ---------------
    def _special_sets(self, allowed_special, disallowed_special):
        if allowed_special == "all":
            allowed_special = set(self._special_tokens)
        if disallowed_special == "all":
            disallowed_special = set(self._special_tokens) - set(allowed_special)
        return set(allowed_special), disallowed_special

    @staticmethod
    def _check_disallowed(text: str, disallowed_special):
        for token in disallowed_special or ():
            if token in text:
                raise ValueError(f"Encountered disallowed special token {token!r}. "
                                 f"Pass it to allowed_special to encode it as a special token.")

    def _norm(self, text):
        """A string (or bytes) through the tokenizer's normalizer: td_nfc_host, the tables the device uses."""
        if self.normalizer is None:
            return text
        data = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else bytes(text)
        out = _capi.nfc_host(data, [0, len(data)])[0].tobytes()
        return out.decode("utf-8", "surrogatepass") if isinstance(text, str) else out

    def _norm_all(self, texts):
        return texts if self.normalizer is None else [self._norm(t) for t in texts]

    def encode_ordinary(self, text: str) -> list[int]:
        text = self._norm(text)
        try:
            return self._core_bpe.encode_ordinary(text)
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def encode(
        self,
        text: str,
        *,
        allowed_special: Literal["all"] | AbstractSet[str] = set(),
        disallowed_special: Literal["all"] | Collection[str] = set(),
    ) -> list[int]:
        allowed, disallowed = self._special_sets(allowed_special, disallowed_special)
        text = self._norm(text)
        self._check_disallowed(text, disallowed)
        try:
            tokens, _ = self._core_bpe.encode(text, allowed)
            return tokens
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def encode_with_special_tokens(self, text: str) -> list[int]:
        text = self._norm(text)
        try:
            return self._core_bpe.encode_with_special_tokens(text)
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def encode_batch(
        self,
        text: Sequence[str],
        *,
        num_threads: int = 8,
        allowed_special: Literal["all"] | AbstractSet[str] = set(),
        disallowed_special: Literal["all"] | Collection[str] = set(),
    ) -> list[list[int]]:
        allowed, disallowed = self._special_sets(allowed_special, disallowed_special)
        texts = text if isinstance(text, (list, tuple)) else list(text)  # (the binding takes a private tuple of the items itself)
        texts = self._norm_all(texts)
        if disallowed:  # (nothing to look for otherwise: the loop alone was 0.2 us per document)
            for t in texts:
                self._check_disallowed(t, disallowed)
        try:
            if allowed:  # every text is cut at its allowed special tokens on the host; all ordinary segments of all
                return self._core_bpe.encode_batch_special(texts, allowed)  # texts run on the GPU as one batch
            return self._core_bpe.encode_batch(texts, MODE_ENCODE)
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def encode_ordinary_batch(self, text: Sequence[str], *, num_threads: int = 8) -> list[list[int]]:
        try:
            return self._core_bpe.encode_batch(self._norm_all(list(text)), MODE_ORDINARY)
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def encode_to_numpy(self, text: str | bytes) -> np.ndarray:
        """tiktoken's array-returning encode: int32 ids without a Python int per token."""
        data = self._norm(text.encode("utf-8") if isinstance(text, str) else bytes(text))
        buf = np.frombuffer(data, dtype=np.uint8)
        try:
            toks, _ = self._core_bpe.encode_batch_numpy(buf, np.asarray([0, len(buf)], dtype=np.int64), MODE_ENCODE)
            return toks
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def encode_batch_to_numpy(self, text: np.ndarray | bytes, offsets: np.ndarray, *, ordinary: bool = False):
        """Bulk form: concatenated UTF-8 bytes + int64 document offsets -> (int32 ids, int64 token offsets)."""
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            return self._core_bpe.encode_batch_numpy(buf, np.asarray(offsets, dtype=np.int64),
                                                     MODE_ORDINARY if ordinary else MODE_ENCODE)
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    # ------------------------------------------------------------------ normalisation ----------
    # The Qwen2 / Qwen2.5 / Qwen3 tokenizers normalise to NFC in front of their split pattern (vocab_io.QWEN2_NORMALIZER).  On the
    # device: a check that proves a document NFC at read speed, and a rewrite of the places where it is not.  Token offsets and
    # everything else computed from byte positions refer to the NORMALISED text; give it to the other bulk methods as it stands.
    def normalize_batch(self, text: np.ndarray | bytes, offsets: np.ndarray, form: str = "NFC") -> NormalizedText:
        """Concatenated UTF-8 bytes + int64 document offsets -> their NFC with its offsets, on the GPU."""
        if form != "NFC":
            raise ValueError(f"form must be 'NFC', not {form!r}")
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            return NormalizedText(*hip.nfc(buf, np.asarray(offsets, dtype=np.int64)))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Normalisation failed: {ex}")

    def encode_batch_to_numpy_normalized(self, text: np.ndarray | bytes, offsets: np.ndarray, *, ordinary: bool = False, return_text: bool = False):
        """encode_batch_to_numpy behind the NFC check: text that is proven NFC is encoded as it lies on the device, anything else is
        normalised there first -> (int32 ids, int64 token offsets), with return_text also a NormalizedText (its flags: None)."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            ids, toff, norm, noff, changed, counts = hip.encode_batch_nfc(buf, np.asarray(offsets, dtype=np.int64),
                                                                          MODE_ORDINARY if ordinary else MODE_ENCODE, return_text=return_text)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return (ids, toff, NormalizedText(norm, noff, None, changed, counts)) if return_text else (ids, toff)

    # ------------------------------------------------------------------ UTF-8 repair -----------
    # The bulk methods take raw bytes; the reference only ever sees str.  On the device: a check at read speed, and
    # bytes.decode("utf-8", errors).encode("utf-8") per document.  Repair comes before normalize_batch when both are wanted.
    def validate_batch(self, text: np.ndarray | bytes, offsets: np.ndarray) -> ValidatedText:
        """Concatenated bytes + int64 document offsets -> which documents are well-formed UTF-8, on the GPU: an upload and the check
        (td_utf8_check_device's kernels, one pass over the text); counts[1] alone is counted."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            _, _, flags, first, _, counts = hip.utf8(buf, np.asarray(offsets, dtype=np.int64), check_only=True)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Validation failed: {ex}")
        return ValidatedText(flags, first, counts)

    def repair_batch(self, text: np.ndarray | bytes, offsets: np.ndarray, errors: str = "replace") -> RepairedText:
        """Concatenated bytes + int64 document offsets -> well-formed UTF-8 with its offsets, on the GPU."""
        policy = _utf8_policy(errors)
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            return RepairedText(*hip.utf8(buf, np.asarray(offsets, dtype=np.int64), policy))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Repair failed: {ex}")

    def encode_batch_to_numpy_repaired(self, text: np.ndarray | bytes, offsets: np.ndarray, *, errors: str = "replace", ordinary: bool = False,
                                       return_text: bool = False):
        """encode_batch_to_numpy behind the UTF-8 check: well-formed text is encoded as it lies on the device, anything else is repaired
        there first -> (int32 ids, int64 token offsets), with return_text also a RepairedText."""
        policy = _utf8_policy(errors)
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            ids, toff, fixed, foff, flags, first, nbad, counts = hip.encode_batch_utf8(buf, np.asarray(offsets, dtype=np.int64),
                                                                                        MODE_ORDINARY if ordinary else MODE_ENCODE, policy,
                                                                                        return_text=return_text)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return (ids, toff, RepairedText(fixed, foff, flags, first, nbad, counts)) if return_text else (ids, toff)

    # ------------------------------------------------------------------ text statistics ---------
    # What the heuristic quality filters (Gopher, C4, FineWeb) threshold, per document, on the device; "local" are the columns one pass
    # over the text gives, "runs" the ones that need to know where a word or a line began.
    def text_stats(self, text: np.ndarray | bytes, offsets: np.ndarray, groups: str = "all") -> TextStats:
        """Concatenated bytes + int64 document offsets -> TextStats, on the GPU."""
        g = _ts_groups(groups)
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            return TextStats(*hip.text_stats(buf, np.asarray(offsets, dtype=np.int64), g))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Text statistics failed: {ex}")

    def encode_batch_to_numpy_with_stats(self, text: np.ndarray | bytes, offsets: np.ndarray, *, ordinary: bool = False):
        """encode_batch_to_numpy and text_stats of one upload -> (int32 ids, int64 token offsets, TextStats)."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            ids, toff, stats, totals = hip.encode_batch_text_stats(buf, np.asarray(offsets, dtype=np.int64),
                                                                   MODE_ORDINARY if ordinary else MODE_ENCODE)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return ids, toff, TextStats(stats, totals)

    # ------------------------------------------------------------------ offsets ----------------
    # The start of a token is where its text begins in its document: in "bytes", the offset of its first UTF-8 byte; in "chars",
    # tiktoken's decode_with_offsets rule (code points; a token that begins inside a character points at that character), which
    # for a str is the index into that str.  Computed on the GPU (include/tokendagger_hip.h, TD_UNIT_*); the end of a token in
    # bytes is its start + len(decode_single_token_bytes(token)).
    @staticmethod
    def _unit(unit: str) -> int:
        if unit not in _UNITS:
            raise ValueError(f"unit must be 'bytes' or 'chars', not {unit!r}")
        return _UNITS[unit]

    def encode_with_offsets(
        self,
        text: str | bytes,
        *,
        allowed_special: Literal["all"] | AbstractSet[str] = set(),
        disallowed_special: Literal["all"] | Collection[str] = set(),
        unit: str | None = None,
    ) -> tuple[list[int], list[int]]:
        """encode() and the start of every token: chars by default for a str, bytes for bytes."""
        is_str = isinstance(text, str)
        u = self._unit(unit or ("chars" if is_str else "bytes"))
        allowed, disallowed = self._special_sets(allowed_special, disallowed_special)
        self._check_disallowed(text if is_str else bytes(text).decode("utf-8", "replace"), disallowed)
        try:
            return self._core_bpe.encode_with_starts(text if is_str else bytes(text), allowed, u)
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def encode_batch_to_numpy_with_offsets(self, text: np.ndarray | bytes, offsets: np.ndarray, *, ordinary: bool = False,
                                           unit: str = "bytes"):
        """encode_batch_to_numpy and the start of every token in its document: -> (int32 ids, int64 token offsets, int64 starts)."""
        u = self._unit(unit)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            return self._core_bpe.encode_batch_numpy_with_starts(buf, np.asarray(offsets, dtype=np.int64),
                                                                 MODE_ORDINARY if ordinary else MODE_ENCODE, u)
        except Exception as e:
            raise TokenDaggerError(f"Encoding failed: {e}")

    def decode_with_offsets(self, tokens: Sequence[int]) -> tuple[str, list[int]]:
        """tiktoken's Encoding.decode_with_offsets: the text (decoded strictly) and the char offset of every token in it."""
        ids = np.asarray(list(tokens), dtype=np.int32)
        try:
            data = self._core_bpe.decode_to_bytes(ids)
            starts = self._core_bpe.token_starts(ids, _UNITS["chars"]).tolist()
        except Exception as e:
            raise TokenDaggerError(f"Decoding failed: {e}")
        return data.decode("utf-8", errors="strict"), starts

    # ------------------------------------------------------------------ training rows ----------
    # Documents -> rows of seq_len ids on the GPU: "concat" packs [BOS] ids [EOS] of every document into one stream cut into rows
    # (cu_seqlens and positions restart at every document and row start), "pad" gives every document a row of its own,
    # truncated to seq_len with its EOS kept.  bos / eos: an id or a special-token string; pad=None: eos, and an error if
    # padding is needed and there is no eos.
    def _rows_args(self, seq_len: int, layout: str, bos, eos, pad):
        if layout not in _LAYOUTS:
            raise ValueError(f"layout must be 'concat' or 'pad', not {layout!r}")

        def tid(x):
            if x is None:
                return -1
            if isinstance(x, (str, bytes)):
                return self.encode_single_token(x)
            return int(x)
        b, e = tid(bos), tid(eos)
        return _LAYOUTS[layout], b, e, (int(pad) if pad is not None else (e if e >= 0 else 0)), pad is None and e < 0

    @staticmethod
    def _rows(r, layout: int, seq_len: int, no_pad: bool) -> Rows:
        ids, pos, aux, counts = r
        if no_pad and int(counts[1]) < int(counts[0]) * seq_len:
            raise ValueError("the rows need padding: pass pad=, or eos= to pad with it")
        return Rows(ids, pos, aux if layout == 0 else None, aux if layout == 1 else None, counts)

    def encode_batch_to_rows(self, text: np.ndarray | bytes, offsets: np.ndarray, seq_len: int, *, layout: str = "concat", bos=None,
                             eos=None, pad=None, drop_last: bool = False, positions: bool = False, cu_seqlens: bool = True,
                             ordinary: bool = False) -> Rows:
        """encode_batch_to_numpy straight into training rows (one call; the ids never leave the device)."""
        lay, b, e, p, no_pad = self._rows_args(seq_len, layout, bos, eos, pad)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            r = self._core_bpe.encode_batch_numpy_rows(buf, np.asarray(offsets, dtype=np.int64), seq_len, lay, b, e, p, drop_last, positions,
                                                       cu_seqlens or lay == 1, MODE_ORDINARY if ordinary else MODE_ENCODE)
        except Exception as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return self._rows(r, lay, seq_len, no_pad)

    def ids_to_rows(self, ids: np.ndarray, tok_offsets: np.ndarray, seq_len: int, *, layout: str = "concat", bos=None, eos=None, pad=None,
                    drop_last: bool = False, positions: bool = False, cu_seqlens: bool = True) -> Rows:
        """Rows from ids already encoded (int32 ids + int64 per-document token offsets, what encode_batch_to_numpy returns)."""
        lay, b, e, p, no_pad = self._rows_args(seq_len, layout, bos, eos, pad)
        try:
            r = self._core_bpe.ids_to_rows(np.asarray(ids, dtype=np.int32), np.asarray(tok_offsets, dtype=np.int64), seq_len, lay, b, e, p,
                                           drop_last, positions, cu_seqlens or lay == 1)
        except Exception as ex:
            raise TokenDaggerError(f"Making rows failed: {ex}")
        return self._rows(r, lay, seq_len, no_pad)

    # Whole documents -> rows by best-fit decreasing: every document stays whole inside one row when it fits ([BOS] ids [EOS]);
    # a longer one is cut at multiples of seq_len (or truncated with its EOS kept, truncate=True) and its last chunk packed like
    # the others.  bos / eos / pad as for ids_to_rows.
    def _packed(self, r, no_pad: bool) -> PackedRows:
        ids, pos, cu, lens, docs, counts = r
        if no_pad and int(counts[1]) < ids.size:
            raise ValueError("the rows need padding: pass pad=, or eos= to pad with it")
        return PackedRows(ids, pos, cu, lens, docs, counts)

    def ids_to_packed_rows(self, ids: np.ndarray, tok_offsets: np.ndarray, seq_len: int, *, bos=None, eos=None, pad=None,
                           truncate: bool = False, positions: bool = False, cu_seqlens: bool = True, docs: bool = False) -> PackedRows:
        """Best-fit-decreasing rows from ids already encoded (int32 ids + int64 per-document token offsets)."""
        _, b, e, p, no_pad = self._rows_args(seq_len, "concat", bos, eos, pad)
        try:
            r = self._core_bpe.ids_to_packed_rows(np.asarray(ids, dtype=np.int32), np.asarray(tok_offsets, dtype=np.int64), seq_len, b, e, p,
                                                  truncate, positions, cu_seqlens, True, docs)
        except Exception as ex:
            raise TokenDaggerError(f"Packing rows failed: {ex}")
        return self._packed(r, no_pad)

    def encode_batch_to_packed_rows(self, text: np.ndarray | bytes, offsets: np.ndarray, seq_len: int, *, bos=None, eos=None, pad=None,
                                    truncate: bool = False, positions: bool = False, cu_seqlens: bool = True, docs: bool = False,
                                    ordinary: bool = False) -> PackedRows:
        """encode_batch_to_numpy straight into best-fit-decreasing rows (one call; the ids never leave the device)."""
        _, b, e, p, no_pad = self._rows_args(seq_len, "concat", bos, eos, pad)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            r = self._core_bpe.encode_batch_numpy_packed_rows(buf, np.asarray(offsets, dtype=np.int64), seq_len, b, e, p, truncate, positions,
                                                              cu_seqlens, True, docs, MODE_ORDINARY if ordinary else MODE_ENCODE)
        except Exception as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return self._packed(r, no_pad)

    # One document per row with every id kept: a document longer than the row's room continues in further rows of its own, each
    # repeating the last `overlap` ids of the row before (Hugging Face: stride + return_overflowing_tokens).  bos / eos / pad as
    # for ids_to_rows; every row gets its own BOS and EOS.
    def _windows(self, r, no_pad: bool) -> WindowRows:
        ids, pos, lens, docs, starts, counts = r
        if no_pad and int(counts[1]) < ids.size:
            raise ValueError("the rows need padding: pass pad=, or eos= to pad with it")
        return WindowRows(ids, pos, lens, docs, starts, counts)

    def ids_to_window_rows(self, ids: np.ndarray, tok_offsets: np.ndarray, seq_len: int, *, overlap: int = 0, bos=None, eos=None, pad=None,
                           positions: bool = False) -> WindowRows:
        """Window rows from ids already encoded (int32 ids + int64 per-document token offsets)."""
        _, b, e, p, no_pad = self._rows_args(seq_len, "pad", bos, eos, pad)
        try:
            r = self._core_bpe.ids_to_window_rows(np.asarray(ids, dtype=np.int32), np.asarray(tok_offsets, dtype=np.int64), seq_len,
                                                  int(overlap), b, e, p, positions, True, True, True)
        except Exception as ex:
            raise TokenDaggerError(f"Making window rows failed: {ex}")
        return self._windows(r, no_pad)

    def encode_batch_to_window_rows(self, text: np.ndarray | bytes, offsets: np.ndarray, seq_len: int, *, overlap: int = 0, bos=None,
                                    eos=None, pad=None, positions: bool = False, ordinary: bool = False) -> WindowRows:
        """encode_batch_to_numpy straight into window rows (one call; the ids never leave the device)."""
        _, b, e, p, no_pad = self._rows_args(seq_len, "pad", bos, eos, pad)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            r = self._core_bpe.encode_batch_numpy_window_rows(buf, np.asarray(offsets, dtype=np.int64), seq_len, int(overlap), b, e, p,
                                                              positions, True, True, True, MODE_ORDINARY if ordinary else MODE_ENCODE)
        except Exception as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return self._windows(r, no_pad)

    # ------------------------------------------------------------------ document selection -----
    # Choose, reorder, repeat and length-filter encoded documents on the device: `order` lists document indices in the order the
    # result is to have them (None: as they are; a shuffle is rng.permutation(n_docs), a split a slice of it, up-sampling a list
    # with repeats), and listed documents with fewer than min_len or more than max_len ids are dropped.  The result is again
    # ids + offsets: feed it to ids_to_rows / ids_to_packed_rows / ids_to_window_rows / ids_to_labeled_rows.
    def select_docs(self, ids: np.ndarray, tok_offsets: np.ndarray, order=None, *, min_len: int = 0, max_len: int | None = None, labels=None):
        """-> (ids, offsets, docs), or (ids, labels, offsets, docs) with a label stream aligned with ids; docs[k]: the input
        document that output document k is."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        try:
            i, l, o, d, _ = hip.select_docs(ids, tok_offsets, order, _capi.select_spec(int(min_len), max_len), labels=labels)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Selecting documents failed: {ex}")
        return (i, o, d) if labels is None else (i, l, o, d)

    def encode_batch_select(self, text: np.ndarray | bytes, offsets: np.ndarray, order=None, *, min_len: int = 0, max_len: int | None = None,
                            ordinary: bool = False):
        """encode_batch_to_numpy and select_docs in one call (the ids never leave the device in between) -> (ids, offsets, docs)."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            i, o, d, _ = hip.encode_batch_select(buf, np.asarray(offsets, dtype=np.int64), order, _capi.select_spec(int(min_len), max_len),
                                                 mode=MODE_ORDINARY if ordinary else MODE_ENCODE)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return i, o, d

    # ------------------------------------------------------------------ field joins ------------
    # One example from several encoded fields (prompt + completion, prompt + chosen / rejected, query + passage, chat turns): the
    # K fields of an example are K documents of the stream, example x's at x * K .. x * K + K - 1 (field_major: field f's at
    # f * n_ex + x).  `fields` has one dict a field, with the keys (all optional)
    #   before        literal ids or special-token strings written in front of the body (the template: never passes through text)
    #   max_len       a cap on the body          shrink_rank   0: never cut for max_total; > 0: cut in ascending rank
    #   keep_tail     a cut body keeps its END   train         the body is trained       train_before   the literals are trained
    #   type          the value of the type stream on the field
    # tail: literals behind the last field.  shrink: "order" (by shrink_rank) or "longest" (Hugging Face's longest_first).  An
    # example that cannot be cut to max_total is dropped.
    def _join_literals(self, items) -> list[int]:
        out = []
        for x in items:
            if isinstance(x, str):
                if x not in self._special_tokens:
                    raise TokenDaggerError(f"{x!r} is not a special token of this vocabulary")
                x = self._special_tokens[x]
            out.append(int(x))
        return out

    def _join_spec(self, fields, tail, tail_type, train_tail, max_total, shrink, field_major, ignore_index):
        known = {"before", "max_len", "shrink_rank", "keep_tail", "train", "train_before", "type"}
        fs = []
        for f in fields:
            if set(f) - known:
                raise TokenDaggerError(f"unknown field keys: {sorted(set(f) - known)}")
            fs.append(_capi.join_field(self._join_literals(f.get("before", ())), f.get("max_len"), f.get("shrink_rank", 0), f.get("type", 0),
                                       bool(f.get("keep_tail", False)), bool(f.get("train", False)), bool(f.get("train_before", False))))
        if shrink not in ("order", "longest"):
            raise TokenDaggerError('shrink must be "order" or "longest"')
        try:
            return _capi.join_spec(fs, self._join_literals(tail), tail_type, train_tail, max_total, shrink, field_major, ignore_index)
        except ValueError as ex:
            raise TokenDaggerError(str(ex))

    def join_fields(self, ids: np.ndarray, tok_offsets: np.ndarray, fields, *, tail=(), max_total: int | None = None, shrink: str = "order",
                    field_major: bool = False, ignore_index: int = -100, labels: bool = True, types: bool = False, tail_type: int = 0,
                    train_tail: bool = False) -> JoinedFields:
        """Examples from fields already encoded (int32 ids + int64 per-document token offsets, len(fields) documents an example)."""
        spec = self._join_spec(fields, tail, tail_type, train_tail, max_total, shrink, field_major, ignore_index)
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        try:
            return JoinedFields(*hip.join_fields(ids, tok_offsets, spec, labels=labels, types=types, field_len=True))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Joining fields failed: {ex}")

    def encode_fields(self, texts_per_field, fields, *, offsets=None, tail=(), max_total: int | None = None, shrink: str = "order",
                      ignore_index: int = -100, labels: bool = True, types: bool = False, tail_type: int = 0, train_tail: bool = False,
                      ordinary: bool = False) -> JoinedFields:
        """Encode and join in one call (the ids never leave the device in between).  texts_per_field: len(fields) equally long
        lists of str / bytes, list f holding field f of every example; or, with offsets=, one bytes / uint8 buffer and its int64
        document offsets, field-major (field f of example x is document f * n_ex + x).  The text is encoded with no special
        token allowed: a field that contains the string of a special token gets that string's ordinary ids."""
        spec = self._join_spec(fields, tail, tail_type, train_tail, max_total, shrink, True, ignore_index)
        if offsets is None:
            lists = [list(col) for col in texts_per_field]
            if len(lists) != len(fields) or len({len(col) for col in lists}) > 1:
                raise TokenDaggerError("texts_per_field needs one list a field, all equally long")
            docs = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for col in lists for s in col]
            buf = np.frombuffer(b"".join(docs), dtype=np.uint8)
            offs = np.concatenate([[0], np.cumsum([len(d) for d in docs], dtype=np.int64)]).astype(np.int64)
        else:
            buf = np.frombuffer(texts_per_field, dtype=np.uint8) if isinstance(texts_per_field, (bytes, bytearray)) else texts_per_field
            offs = np.asarray(offsets, dtype=np.int64)
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        try:
            return JoinedFields(*hip.encode_batch_join(buf, offs, spec, mode=MODE_ORDINARY if ordinary else MODE_ENCODE, labels=labels,
                                                       types=types, field_len=True))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")

    # ------------------------------------------------------------------ token counts -----------
    # What is in the ids: counts[g, v] = how often id v occurs in the documents of group g (a source, a language, a split), on the
    # device.  Any int32 stream aligned with ids counts as well: ids_to_counts(labels) is the histogram of the TRAINED tokens, the
    # ignore_index shows in `negative`.  Counts add: out= accumulates over calls, dist.sum_counts over ranks.
    def _counts_args(self, tok_offsets, groups, n_groups, n_bins, out, strict):
        n_bins = self.n_vocab if n_bins is None else int(n_bins)
        if groups is None:
            if n_groups not in (None, 1):
                raise TokenDaggerError("n_groups needs groups")
            n_groups, g = 1, None
        else:
            if tok_offsets is None:
                raise TokenDaggerError("groups needs tok_offsets")
            g = np.ascontiguousarray(groups, dtype=np.int32)
            n_groups = int(n_groups) if n_groups is not None else (int(g.max()) + 1 if g.size else 1)
            # (one group is the contract's form without documents: the groups are checked here, the offsets bound nothing new)
        if out is not None:
            want = (n_bins,) if groups is None else (n_groups, n_bins)
            if not isinstance(out, np.ndarray) or out.dtype != np.int64 or out.shape != want or not out.flags.c_contiguous:
                raise TokenDaggerError(f"out must be a contiguous int64 array of shape {want}")
        # (strict: the call counts into an array of its own, and `out` is added to only behind the check: a raise leaves it as it was)
        direct = out is not None and not strict
        spec = _capi.counts_spec(n_bins, n_groups, accumulate=direct)
        return g, spec, (out.reshape(-1) if direct else None)

    @staticmethod
    def _counts_result(counts, info, grouped: bool, out, strict: bool):
        if strict and int(info[2]) > 0:
            raise TokenDaggerError(f"{int(info[2])} ids are at or above n_bins: these are not this vocabulary's ids (strict=False counts the rest)")
        if out is not None and strict:
            out += counts.reshape(out.shape)
        c = out if out is not None else (counts if grouped else counts.reshape(-1))
        return c, int(info[0]), int(info[1]), int(info[2])

    def ids_to_counts(self, ids: np.ndarray, tok_offsets: np.ndarray | None = None, *, groups=None, n_groups: int | None = None,
                      n_bins: int | None = None, out: np.ndarray | None = None, strict: bool = True) -> TokenCounts:
        """Histogram of ids (n_bins: default n_vocab), per group of documents where groups[n_docs] is given (n_groups: default
        max(groups) + 1).  out=: an int64 array of the result's shape that is added to.  strict: ids >= n_bins raise, and `out` is then left as it was."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        g, spec, flat = self._counts_args(tok_offsets, groups, n_groups, n_bins, out, strict)
        if g is not None and spec.n_groups == 1:
            if g.size and (g.min() < 0 or g.max() > 0):
                raise TokenDaggerError("Counting tokens failed: a group is outside [0, n_groups)")
            o = np.asarray(tok_offsets, dtype=np.int64)
            ids, tok_offsets, g = np.asarray(ids, dtype=np.int32)[int(o[0]):int(o[-1])], None, None
        try:
            counts, info = hip.token_counts(ids, tok_offsets if g is not None else None, g, spec, counts=flat)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Counting tokens failed: {ex}")
        return TokenCounts(*self._counts_result(counts, info, groups is not None, out, strict))

    def encode_batch_to_counts(self, text: np.ndarray | bytes, offsets: np.ndarray, *, groups=None, n_groups: int | None = None,
                               n_bins: int | None = None, out: np.ndarray | None = None, strict: bool = True,
                               ordinary: bool = False) -> EncodedTokenCounts:
        """encode_batch_to_numpy and ids_to_counts in one call: the ids never leave the device, only the counts come back."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        g, spec, flat = self._counts_args(offsets, groups, n_groups, n_bins, out, strict)
        if g is not None and spec.n_groups == 1 and g.size and (g.min() < 0 or g.max() > 0):
            raise TokenDaggerError("Counting tokens failed: a group is outside [0, n_groups)")
        try:
            counts, info, total = hip.encode_batch_token_counts(buf, np.asarray(offsets, dtype=np.int64), g if spec.n_groups > 1 else None, spec,
                                                                mode=MODE_ORDINARY if ordinary else MODE_ENCODE, counts=flat)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return EncodedTokenCounts(*self._counts_result(counts, info, groups is not None, out, strict), total)

    # ------------------------------------------------------------------ n-gram matches ---------
    # "Does this document contain any of these known token sequences?" on the device: decontamination against an evaluation set
    # (ngram_set_from_texts(benchmark, 13), then select_docs(ids, tok_offsets, np.flatnonzero(doc_stats[:, 0] == 0))), phrase
    # blocklists, masking the covered ids of a label stream (labels=...).  A set holds up to 2^24 sequences of 1 .. 64 ids in at most 8
    # distinct lengths; use it as a context manager or close() it when the work that uses it is done.
    def ngram_set(self, sequences, offsets=None):
        """A set of id sequences on this tokenizer's device: a list of id lists, or flat ids with offsets[n_pats + 1]."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        try:
            return hip.ngram_set(sequences, offsets)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Building the n-gram set failed: {ex}")

    def ngram_set_from_texts(self, texts: Sequence[str], n: int, stride: int = 1):
        """Every n-gram (n ids) of every text, at every stride-th position, de-duplicated: the decontamination recipe.  Texts shorter
        than n ids contribute nothing."""
        if n < 1 or n > _capi.TD_NGRAM_MAX_LEN or stride < 1:
            raise TokenDaggerError("n must be in 1 .. 64 and stride at least 1")
        grams = [np.lib.stride_tricks.sliding_window_view(np.asarray(t, dtype=np.int32), n)[::stride]
                 for t in self.encode_ordinary_batch(list(texts)) if len(t) >= n]
        if not grams:
            raise TokenDaggerError(f"no text has {n} ids: the set would be empty")
        uniq = np.unique(np.concatenate(grams), axis=0)
        return self.ngram_set(uniq.reshape(-1), np.arange(len(uniq) + 1, dtype=np.int64) * n)

    def ids_to_ngram_matches(self, ids: np.ndarray, tok_offsets: np.ndarray, nset, *, cover: bool = True, labels=None,
                             ignore_index: int = -100, pattern_counts: bool = False) -> NgramMatches:
        """Where the sequences of `nset` occur in the documents.  labels: a stream aligned with ids (the ids themselves, or the labels
        of ids_to_labels); a copy comes back with ignore_index at every covered id."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        try:
            return NgramMatches(*hip.ngram_matches(nset, ids, tok_offsets, _capi.ngram_spec(ignore_index), cover=cover, labels=labels,
                                                   pattern_counts=pattern_counts))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Matching n-grams failed: {ex}")

    def encode_batch_to_ngram_matches(self, text: np.ndarray | bytes, offsets: np.ndarray, nset, *, pattern_counts: bool = False,
                                      ordinary: bool = False):
        """encode_batch_to_numpy and ids_to_ngram_matches in one call: the ids never leave the device -> (NgramMatches without cover
        and labels, the ids made)."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            ds, pc, counts, total = hip.encode_batch_ngram_matches(buf, np.asarray(offsets, dtype=np.int64), nset,
                                                                   mode=MODE_ORDINARY if ordinary else MODE_ENCODE, pattern_counts=pattern_counts)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return NgramMatches(None, None, ds, pc, counts), total

    # ------------------------------------------------------------------ MinHash signatures -----
    # Near-duplicate detection's device half: a signature per document over its shingles of `ngram` ids, and with bands > 0 the LSH
    # band keys.  Both are a function of one document, so results of different batches, calls and ranks go side by side; grouping the
    # candidates and choosing the survivors is the caller's (band keys -> np.unique per band -> similarity ->
    # select_docs).  bands b and rows r make two documents of Jaccard similarity s candidates with probability 1 - (1 - s^r)^b;
    # the curve's threshold is about (1 / b)^(1 / r).
    def ids_to_minhash(self, ids: np.ndarray, tok_offsets: np.ndarray, *, ngram: int = 5, num_perm: int = 128, seed: int = 1,
                       bands: int = 0, rows: int | None = None) -> MinHashes:
        """MinHash signatures (and band keys) of encoded documents.  rows=None: num_perm // bands.  ids are not checked against the
        vocabulary: a label stream may be sketched as well."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        try:
            return MinHashes(*hip.minhash(ids, tok_offsets, _capi.minhash_spec(ngram, num_perm, seed, bands, rows)))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"MinHash failed: {ex}")

    def encode_batch_to_minhash(self, text: np.ndarray | bytes, offsets: np.ndarray, *, ngram: int = 5, num_perm: int = 128, seed: int = 1,
                                bands: int = 0, rows: int | None = None, ordinary: bool = False):
        """encode_batch_to_numpy and ids_to_minhash in one call: the ids never leave the device -> (MinHashes, the ids made)."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            sig, keys, counts, total = hip.encode_batch_minhash(buf, np.asarray(offsets, dtype=np.int64),
                                                                _capi.minhash_spec(ngram, num_perm, seed, bands, rows),
                                                                mode=MODE_ORDINARY if ordinary else MODE_ENCODE)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")
        return MinHashes(sig, keys, counts), total

    # ------------------------------------------------------------------ loss labels ------------
    # labels[i] = ids[i] inside a span, ignore_index elsewhere.  A span starts behind an opener (a string, encoded once with every
    # special token allowed, or a list of ids: at most 8 openers of at most 8 ids) and ends with a closer (a special-token string
    # or an id: at most 16), which is trained itself unless train_close=False.  For Llama-4 chat data:
    # open=["<|header_start|>assistant<|header_end|>"], close=["<|eot|>", "<|eom|>"].  Rows of labels: ids_to_rows /
    # ids_to_packed_rows / ids_to_window_rows on `labels` with the same tok_offsets, pad=ignore_index and no bos / eos.
    def _labels_spec(self, open, close, ignore_index: int, train_close: bool):
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        openers = []
        for o in open:
            if isinstance(o, (str, bytes)):
                text = o if isinstance(o, str) else bytes(o).decode("utf-8")
                ids = [int(i) for i in hip.encode_with_special_strs(text.encode("utf-8"), list(self._special_tokens))[0]]
                if len(ids) > _capi.TD_LABELS_MAX_OPEN_LEN:
                    raise ValueError(f"opener {o!r} encodes to {len(ids)} ids: an opener holds at most {_capi.TD_LABELS_MAX_OPEN_LEN}")
                if not ids:
                    raise ValueError("an opener must not be empty")
                openers.append(ids)
            else:
                openers.append([int(i) for i in o])
        closers = [self.encode_single_token(c) if isinstance(c, (str, bytes)) else int(c) for c in close]
        return hip, _capi.labels_spec(openers, closers, ignore_index, train_close)

    def ids_to_labels(self, ids: np.ndarray, tok_offsets: np.ndarray, *, open, close, ignore_index: int = -100, train_close: bool = True,
                      mask: bool = False, trained_offsets: bool = False) -> Labels:
        """Loss labels from ids already encoded (int32 ids + int64 per-document token offsets)."""
        hip, spec = self._labels_spec(open, close, ignore_index, train_close)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        offs = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        try:
            lab, m, to, counts = hip.span_labels(ids, offs, spec, mask=mask, trained_offsets=trained_offsets)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Making labels failed: {ex}")
        return Labels(ids[:len(lab)], offs, lab, m, to, counts)

    def encode_batch_to_labels(self, text: np.ndarray | bytes, offsets: np.ndarray, *, allowed_special: Literal["all"] | AbstractSet[str] = "all",
                               open, close, ignore_index: int = -100, train_close: bool = True, mask: bool = False,
                               trained_offsets: bool = False) -> Labels:
        """Chat text straight to ids + labels (one call): the allowed special tokens are cut out, the ids labelled on the device."""
        hip, spec = self._labels_spec(open, close, ignore_index, train_close)
        allowed = sorted(self._special_tokens) if allowed_special == "all" else sorted(allowed_special)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        try:
            return Labels(*hip.encode_batch_span_labels(buf, np.asarray(offsets, dtype=np.int64), allowed, spec, mask=mask,
                                                        trained_offsets=trained_offsets))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")

    # ------------------------------------------------------------------ loss labels from byte ranges ---
    # For data whose trained regions are known as offsets into the text (plain-text templates, prompt / completion pairs, field
    # values): per document a sorted list of disjoint half-open byte ranges, relative to the document's first byte.  `ranges` is
    # (range_offsets, array[n, 2]) or one sequence of (begin, end) per document.  rule: "overlap" trains an id with any marked byte,
    # "inside" one whose bytes are all marked, "start" one whose first byte is marked.  counts[1] is the number of ids that straddle
    # an edge of a range.  unit="chars" (the text forms only): the ranges count code points; they are converted to bytes on the
    # host, one numpy pass over the text, before the call.
    def _range_args(self, rule, ignore_index: int):
        return _capi.HipTokenizer.borrow(self._core_bpe.handle()), _capi.range_spec(rule, ignore_index)

    @staticmethod
    def _text_ranges(buf, offs, ranges, unit: str):
        if unit not in ("bytes", "chars"):
            raise ValueError("unit must be 'bytes' or 'chars'")
        return _capi.chars_to_bytes(buf, offs, ranges) if unit == "chars" else _capi.as_ranges(ranges, len(offs) - 1)

    def ids_to_range_labels(self, ids: np.ndarray, tok_offsets: np.ndarray, ranges, *, rule: str = "overlap", ignore_index: int = -100,
                            mask: bool = False, trained_offsets: bool = False, starts=None) -> Labels:
        """Loss labels from ids already encoded and byte ranges.  starts None: every document's bytes are its ids' bytes
        concatenated; else int64 byte starts per id (encode_batch_to_numpy_with_offsets), for patterns that skip text."""
        hip, spec = self._range_args(rule, ignore_index)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        offs = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        try:
            lab, m, to, counts = hip.range_labels(ids, offs, ranges, spec, mask=mask, trained_offsets=trained_offsets, starts=starts)
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Making labels failed: {ex}")
        return Labels(ids[:len(lab)], offs, lab, m, to, counts)

    def encode_batch_to_range_labels(self, text: np.ndarray | bytes, offsets: np.ndarray, ranges, *, rule: str = "overlap", unit: str = "bytes",
                                     allowed_special: Literal["all"] | AbstractSet[str] = "all", ignore_index: int = -100, mask: bool = False,
                                     trained_offsets: bool = False) -> Labels:
        """Text and ranges into it straight to ids + labels (one call): the ids are labelled on the device where the encode leaves them."""
        hip, spec = self._range_args(rule, ignore_index)
        allowed = sorted(self._special_tokens) if allowed_special == "all" else sorted(allowed_special)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        offs = np.asarray(offsets, dtype=np.int64)
        rg = self._text_ranges(buf, offs, ranges, unit)
        try:
            return Labels(*hip.encode_batch_range_labels(buf, offs, allowed, rg, spec, mask=mask, trained_offsets=trained_offsets))
        except _capi.TokenDaggerHipError as ex:
            raise TokenDaggerError(f"Encoding failed: {ex}")

    # ------------------------------------------------------------------ label rows -------------
    # (input_ids, labels) rows in one pass: `labels` is a stream index-aligned with the ids (ids_to_labels gives one) and is placed by
    # the placement of the ids.  Where the id rows hold the inserted BOS / EOS / a pad slot the label rows hold label_bos /
    # label_eos (None: the EOS id itself, so that the model learns to stop) / label_pad.  mask_overlap (windows): the ids a window
    # repeats from the one before are label_pad, so every id is trained in exactly one row.
    _ROW_LAYOUTS = {"concat": 0, "pad": 1, "bestfit": 2, "windows": 3}

    def _labeled_args(self, seq_len, layout, bos, eos, pad, label_bos, label_eos, label_pad, overlap, mask_overlap, drop_last, truncate):
        if layout not in self._ROW_LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(self._ROW_LAYOUTS)}, not {layout!r}")
        if mask_overlap and layout != "windows":
            raise ValueError("mask_overlap is for layout='windows'")
        if overlap and layout != "windows":
            raise ValueError("overlap is for layout='windows'")
        if drop_last and layout != "concat":
            raise ValueError("drop_last is for layout='concat'")
        if truncate and layout != "bestfit":
            raise ValueError("truncate is for layout='bestfit'")
        _, b, e, p, no_pad = self._rows_args(seq_len, "concat", bos, eos, pad)
        lay = self._ROW_LAYOUTS[layout]
        flags = (_capi.TD_ROWS_DROP_LAST if drop_last else 0) | (_capi.TD_ROWS_TRUNCATE if truncate else 0)
        le = int(label_eos) if label_eos is not None else (e if e >= 0 else int(label_pad))
        return lay, b, e, p, no_pad, flags, int(label_bos), le, int(label_pad), _capi.TD_ROWLAB_MASK_OVERLAP if mask_overlap else 0

    def _labeled(self, lay: int, seq_len: int, no_pad: bool, r) -> LabeledRows:
        *head, lab = r
        rows = self._rows(head, lay, seq_len, no_pad) if lay < 2 else self._packed(head, no_pad) if lay == 2 else self._windows(head, no_pad)
        return LabeledRows(rows, lab)

    def ids_to_labeled_rows(self, ids: np.ndarray, labels: np.ndarray, tok_offsets: np.ndarray, seq_len: int, *, layout: str = "concat",
                            bos=None, eos=None, pad=None, label_bos: int = -100, label_eos=None, label_pad: int = -100, overlap: int = 0,
                            mask_overlap: bool = False, drop_last: bool = False, truncate: bool = False, positions: bool = False,
                            cu_seqlens: bool = True, docs: bool = False) -> LabeledRows:
        """Id rows and label rows from ids already encoded and a label stream aligned with them (one call, one pass)."""
        lay, b, e, p, no_pad, flags, lb, le, lp, lflags = self._labeled_args(seq_len, layout, bos, eos, pad, label_bos, label_eos, label_pad,
                                                                              overlap, mask_overlap, drop_last, truncate)
        try:
            r = self._core_bpe.ids_to_labeled_rows(np.asarray(ids, dtype=np.int32), np.asarray(labels, dtype=np.int32),
                                                   np.asarray(tok_offsets, dtype=np.int64), seq_len, lay, int(overlap), b, e, p, flags, lb, le, lp,
                                                   lflags, positions, cu_seqlens or lay == 1, True, docs or lay == 3, True)
        except Exception as ex:
            raise TokenDaggerError(f"Making labeled rows failed: {ex}")
        return self._labeled(lay, seq_len, no_pad, r)

    def encode_batch_to_labeled_rows(self, text: np.ndarray | bytes, offsets: np.ndarray, seq_len: int, *, layout: str = "concat", open, close,
                                     allowed_special: Literal["all"] | AbstractSet[str] = "all", ignore_index: int = -100,
                                     train_close: bool = True, bos=None, eos=None, pad=None, label_bos=None, label_eos=None, label_pad=None,
                                     overlap: int = 0, mask_overlap: bool = False, drop_last: bool = False, truncate: bool = False,
                                     positions: bool = False, cu_seqlens: bool = True, docs: bool = False) -> LabeledRows:
        """Chat text straight to id rows and label rows (one call): encode_batch_to_labels then ids_to_labeled_rows, with the ids and
        the labels staying on the device in between.  label_bos / label_pad default to ignore_index.  The exception of a capacity
        error carries .counts (counts[0]: the rows needed)."""
        hip, lspec = self._labels_spec(open, close, ignore_index, train_close)
        lay, b, e, p, no_pad, flags, lb, le, lp, lflags = self._labeled_args(
            seq_len, layout, bos, eos, pad, ignore_index if label_bos is None else label_bos, label_eos,
            ignore_index if label_pad is None else label_pad, overlap, mask_overlap, drop_last, truncate)
        allowed = sorted(self._special_tokens) if allowed_special == "all" else sorted(allowed_special)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        rspec = _capi.RowsSpec(lay, seq_len, b, e, p, flags)
        lab = _capi.rows_labels(0, 0, lb, le, lp, flags=lflags)
        try:
            r = hip.encode_batch_span_label_rows(buf, np.asarray(offsets, dtype=np.int64), allowed, lspec, rspec, lab, overlap=int(overlap),
                                                 positions=positions, aux=cu_seqlens or lay == 1, lengths=True, docs=docs or lay == 3,
                                                 starts=True)
        except _capi.TokenDaggerHipError as ex:
            err = TokenDaggerError(f"Encoding failed: {ex}")
            err.counts = getattr(ex, "counts", None)
            raise err
        return self._labeled(lay, seq_len, no_pad, r[:-1])

    def encode_batch_to_range_labeled_rows(self, text: np.ndarray | bytes, offsets: np.ndarray, ranges, seq_len: int, *, layout: str = "concat",
                                           rule: str = "overlap", unit: str = "bytes",
                                           allowed_special: Literal["all"] | AbstractSet[str] = "all", ignore_index: int = -100, bos=None,
                                           eos=None, pad=None, label_bos=None, label_eos=None, label_pad=None, overlap: int = 0,
                                           mask_overlap: bool = False, drop_last: bool = False, truncate: bool = False,
                                           positions: bool = False, cu_seqlens: bool = True, docs: bool = False) -> LabeledRows:
        """encode_batch_to_labeled_rows with byte ranges in place of id spans: encode_batch_to_range_labels then ids_to_labeled_rows,
        with the ids and the labels staying on the device in between."""
        hip, rgspec = self._range_args(rule, ignore_index)
        lay, b, e, p, no_pad, flags, lb, le, lp, lflags = self._labeled_args(
            seq_len, layout, bos, eos, pad, ignore_index if label_bos is None else label_bos, label_eos,
            ignore_index if label_pad is None else label_pad, overlap, mask_overlap, drop_last, truncate)
        allowed = sorted(self._special_tokens) if allowed_special == "all" else sorted(allowed_special)
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        offs = np.asarray(offsets, dtype=np.int64)
        rg = self._text_ranges(buf, offs, ranges, unit)
        rspec = _capi.RowsSpec(lay, seq_len, b, e, p, flags)
        lab = _capi.rows_labels(0, 0, lb, le, lp, flags=lflags)
        try:
            r = hip.encode_batch_range_label_rows(buf, offs, allowed, rg, rgspec, rspec, lab, overlap=int(overlap), positions=positions,
                                                  aux=cu_seqlens or lay == 1, lengths=True, docs=docs or lay == 3, starts=True)
        except _capi.TokenDaggerHipError as ex:
            err = TokenDaggerError(f"Encoding failed: {ex}")
            err.counts = getattr(ex, "counts", None)
            raise err
        return self._labeled(lay, seq_len, no_pad, r[:-1])

    # ------------------------------------------------------------------ decoding ---------------
    def decode_bytes(self, tokens: Sequence[int]) -> bytes:
        try:
            return self._core_bpe.decode_to_bytes(np.asarray(list(tokens), dtype=np.int32))
        except Exception as e:
            raise TokenDaggerError(f"Decoding failed: {e}")

    def decode(self, tokens: Sequence[int], errors: str = "replace") -> str:
        try:
            return self.decode_bytes(tokens).decode("utf-8", errors=errors)
        except TokenDaggerError:
            raise
        except Exception as e:
            raise TokenDaggerError(f"Decoding failed: {e}")

    def decode_batch(self, tokens: Sequence[Sequence[int]], *, num_threads: int = 8, errors: str = "replace") -> list[str]:
        """All documents in one device pass (reference: a thread pool of decode calls, wrapper.py:237-256)."""
        try:
            return [b.decode("utf-8", errors=errors) for b in self._core_bpe.decode_batch([list(t) for t in tokens])]
        except Exception as e:
            raise TokenDaggerError(f"Decoding failed: {e}")

    # ------------------------------------------------------------------ decode rows ------------
    # ids in segments back to text on the device (the contract: include/tokendagger_hip.h, td_decode_spec): a generated [B, S] batch
    # (skip pad and BOS, stop at EOS: Hugging Face's batch_decode(skip_special_tokens=True)), PAD / WINDOWS rows with their lengths,
    # cu_seqlens, a label stream (skip_negative: the text a model is trained on).
    def decode_rows_to_numpy(self, ids: np.ndarray, *, tok_offsets: np.ndarray | None = None, lengths=None, skip_special_tokens: bool = False,
                             skip=(), stop=(), keep_stop: bool = False, skip_negative: bool = False) -> DecodedRows:
        """-> DecodedRows(data uint8[n], offsets int64[n_segs + 1], seg_ids int64[n_segs], n_emitted, n_skipped, n_stopped).  ids: 2-D
        (one segment a row, lengths: the rows' real lengths) or 1-D with tok_offsets.  An id of `stop` ends its segment (and is emitted
        with keep_stop); seg_ids are the ids each segment consumed, the stop id included."""
        hip = _capi.HipTokenizer.borrow(self._core_bpe.handle())
        a = np.asarray(ids)
        if a.ndim == 2:
            if tok_offsets is not None:
                raise TokenDaggerError("tok_offsets goes with 1-D ids; rows take lengths")
            if a.shape[1] == 0:
                return DecodedRows(np.zeros(0, dtype=np.uint8), np.zeros(a.shape[0] + 1, dtype=np.int64), np.zeros(a.shape[0], dtype=np.int64), 0, 0, 0)
            stride, n_segs = int(a.shape[1]), int(a.shape[0])
        elif a.ndim == 1 and tok_offsets is not None:
            if lengths is not None:
                raise TokenDaggerError("lengths goes with 2-D ids")
            stride, n_segs = 0, None
        else:
            raise TokenDaggerError("ids must be 2-D (rows), or 1-D with tok_offsets")
        try:
            spec = _capi.decode_spec(stride, skip, stop, keep_stop=keep_stop, skip_negative=skip_negative, skip_special=skip_special_tokens)
            data, offs, seg, info = hip.decode_rows(a, spec, tok_offsets=tok_offsets, lengths=lengths, n_segs=n_segs)
        except (_capi.TokenDaggerHipError, ValueError, OverflowError) as ex:
            raise TokenDaggerError(f"Decoding failed: {ex}")
        return DecodedRows(np.frombuffer(data, dtype=np.uint8), offs, seg, int(info[1]), int(info[2]), int(info[3]))

    def decode_rows(self, ids: np.ndarray, *, tok_offsets: np.ndarray | None = None, lengths=None, skip_special_tokens: bool = False,
                    skip=(), stop=(), keep_stop: bool = False, skip_negative: bool = False, errors: str = "replace") -> list[str]:
        """One string per segment; the arguments of decode_rows_to_numpy."""
        r = self.decode_rows_to_numpy(ids, tok_offsets=tok_offsets, lengths=lengths, skip_special_tokens=skip_special_tokens, skip=skip,
                                      stop=stop, keep_stop=keep_stop, skip_negative=skip_negative)
        data, o = r.data.tobytes(), r.offsets
        return [data[int(o[d]):int(o[d + 1])].decode("utf-8", errors=errors) for d in range(len(o) - 1)]

    def decode_bytes_batch(self, tokens: Sequence[Sequence[int]]) -> list[bytes]:
        try:
            return self._core_bpe.decode_batch([list(t) for t in tokens])
        except Exception as e:
            raise TokenDaggerError(f"Decoding failed: {e}")

    def decode_single_token_bytes(self, token: int) -> bytes:
        """tiktoken semantics: KeyError for an id that is not in the vocabulary (host table lookup, no launch)."""
        b = self._core_bpe.token_bytes(int(token))
        if b is None:
            raise KeyError(token)
        return b

    def decode_tokens_bytes(self, tokens: Sequence[int]) -> list[bytes]:
        return [self.decode_single_token_bytes(t) for t in tokens]

    def encode_single_token(self, text_or_bytes: str | bytes) -> int:
        """tiktoken semantics: the id of exactly one token (ordinary or special), KeyError otherwise."""
        data = text_or_bytes.encode("utf-8") if isinstance(text_or_bytes, str) else bytes(text_or_bytes)
        tid = self._core_bpe.single_token(data)
        if tid is None:
            raise KeyError(text_or_bytes)
        return tid

    def token_byte_values(self) -> list[bytes]:
        """Byte strings of all ordinary tokens, sorted (tiktoken.Encoding.token_byte_values)."""
        special = set(self._special_tokens.values())
        out = []
        for t in range(self.max_token_value + 1):
            if t in special:
                continue
            b = self._core_bpe.token_bytes(t)
            if b is not None:
                out.append(b)
        return sorted(out)

    @property
    def eot_token(self) -> int:
        return self._special_tokens["<|endoftext|>"]

    # ------------------------------------------------------------------ utilities --------------
    def special_tokens(self) -> list[str]:
        try:
            return self._core_bpe.special_tokens()
        except Exception as e:
            raise TokenDaggerError(f"Failed to get special tokens: {e}")

    @property
    def special_tokens_set(self) -> set[str]:
        return set(self._special_tokens)

    @property
    def n_vocab(self) -> int:
        return self.max_token_value + 1

    def is_special_token(self, token: int) -> bool:
        return token in self._special_tokens.values()


def load_tokenizer(name: str, vocab_file: str | Path, pattern: str, special_tokens_file: str | Path | None = None) -> Tokenizer:
    """Reference: wrapper.py:333-355.  The JSON files are read by the C++ loader (td_vocab_load_json)."""
    return Tokenizer.from_files(name, pat_str=pattern, vocab_file=vocab_file, special_tokens_file=special_tokens_file)


def load_tiktoken_bpe(path: str | Path) -> dict[bytes, int]:
    """``tiktoken.load.load_tiktoken_bpe`` for a local ``.model`` / ``.tiktoken`` file (C++ loader)."""
    from . import capi
    return capi.load_tiktoken_bpe(path)


def create_tokenizer(name: str, pattern: str, vocab: list[dict], special_tokens: dict[str, int] | None = None) -> Tokenizer:
    return Tokenizer(name=name, pattern=pattern, vocab=vocab, special_tokens=special_tokens)


def Encoding(name: str, *, pat_str: str, mergeable_ranks: dict[bytes, int],
             special_tokens: dict[str, int] | None = None, normalizer: str | None = None) -> Tokenizer:
    """tiktoken-compatible factory (reference: wrapper.py:382-395)."""
    return Tokenizer(name=name, pat_str=pat_str, mergeable_ranks=mergeable_ranks, special_tokens=special_tokens or {}, normalizer=normalizer)


def llama4_scout(device: int = -1) -> Tokenizer:
    """The Llama-4-Scout tokenizer from the bundled TDV1 vocabulary (tokendagger_amd/data)."""
    from . import vocab_io
    name, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    return Tokenizer(name, pat_str=pat, mergeable_ranks=ranks, special_tokens=special, device=device)
