"""Two independent statements of the decode-rows contract (include/tokendagger_hip.h, td_decode_spec) and a generator of random
cases.  Both take the same arguments and return (bytes, out_offsets int64[n_segs + 1], seg_ids int64[n_segs], info int64[4] = bytes,
ids emitted, ids skipped, segments stopped), or raise DecodeError(code, pos): decode_brute walks every segment over a dict of token
bytes, decode_numpy repeats the segments over their positions and uses a segmented cumulative "stopped"."""
import numpy as np

E_INVALID, E_BAD_TOKEN = 1, 8  # (checked against capi's in test_decode_rows_model.py)


class DecodeError(Exception):
    def __init__(self, code, pos):
        super().__init__(f"code {code} at {pos}")
        self.code, self.pos = code, pos


def check_args(n_tokens, tok_offsets=None, row_stride=0, lengths=None, n_segs=None, skip=(), stop=()):
    """The argument errors of the contract -> (n_segs, position of the first error or None)."""
    for i, x in enumerate(list(skip) + list(stop)):
        if x < 0:
            return n_segs, i
    if row_stride == 0:
        o = [int(x) for x in tok_offsets]
        n = len(o) - 1
        if o[0] < 0:
            return n, 0
        for d in range(n):
            if o[d + 1] < o[d]:
                return n, d
        return n, (n if o[n] > n_tokens else None)
    n = n_segs if lengths is None else len(lengths)
    if n * row_stride > n_tokens:
        return n, -1
    if lengths is not None:
        for r, x in enumerate(lengths):
            if not 0 <= x <= row_stride:
                return n, r
    return n, None


def _segments(ids, tok_offsets, row_stride, lengths, n_segs):
    """-> [(first position, length)] of the segments; the arguments are valid."""
    if row_stride == 0:
        o = [int(x) for x in tok_offsets]
        return [(o[d], o[d + 1] - o[d]) for d in range(len(o) - 1)]
    n = n_segs if lengths is None else len(lengths)
    return [(r * row_stride, row_stride if lengths is None else int(lengths[r])) for r in range(n)]


def decode_brute(ids, tok, tok_offsets=None, row_stride=0, lengths=None, n_segs=None, skip=(), stop=(), keep_stop=False,
                 skip_negative=False, skip_special=False, special_ids=()):
    """A plain loop.  tok: dict id -> bytes (special tokens with their literal)."""
    ids = [int(x) for x in np.asarray(ids)]
    n, bad = check_args(len(ids), tok_offsets, row_stride, lengths, n_segs, skip, stop)
    if bad is not None:
        raise DecodeError(E_INVALID, bad)
    skip_set = set(int(x) for x in skip) | (set(int(x) for x in special_ids) if skip_special else set())
    stop_set = set(int(x) for x in stop)
    out, offs, seg_ids, info, first_bad = bytearray(), [0], [], [0, 0, 0, 0], None
    for first, length in _segments(ids, tok_offsets, row_stride, lengths, n_segs):
        consumed = 0
        for i in range(first, first + length):
            x = ids[i]
            consumed += 1
            piece = None  # None: emits nothing, and that is right
            if x < 0:
                if not skip_negative:
                    first_bad = i if first_bad is None else min(first_bad, i)
            else:
                stops = x in stop_set
                if x in skip_set or (stops and not keep_stop):
                    pass
                elif x in tok:
                    piece = tok[x]
                else:
                    first_bad = i if first_bad is None else min(first_bad, i)
                if piece is not None:
                    out += piece
                    info[1] += 1
                else:
                    info[2] += 1
                if stops:
                    info[3] += 1
                    break
                continue
            info[2] += 1  # (a negative id: skipped, or the error below)
        seg_ids.append(consumed)
        offs.append(len(out))
    if first_bad is not None:
        raise DecodeError(E_BAD_TOKEN, first_bad)
    info[0] = len(out)
    return bytes(out), np.asarray(offs, dtype=np.int64), np.asarray(seg_ids, dtype=np.int64), np.asarray(info, dtype=np.int64)


class Vocab:
    """The dict as arrays: lens[id] (0: no token), the bytes of all tokens and where each begins."""

    def __init__(self, tok):
        self.tok = tok
        self.max_id = max(tok) if tok else -1
        self.lens = np.zeros(self.max_id + 1, dtype=np.int64)
        for i, b in tok.items():
            self.lens[i] = len(b)
        self.begin = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.blob = np.frombuffer(b"".join(tok.get(i, b"") for i in range(self.max_id + 1)), dtype=np.uint8)


def decode_numpy(ids, vocab, tok_offsets=None, row_stride=0, lengths=None, n_segs=None, skip=(), stop=(), keep_stop=False,
                 skip_negative=False, skip_special=False, special_ids=()):
    """Vectorised: np.repeat of the segments, a segmented cumulative "stopped", lengths and cumsum."""
    ids = np.asarray(ids, dtype=np.int64)
    skip, stop = np.asarray(list(skip), dtype=np.int64), np.asarray(list(stop), dtype=np.int64)
    if (skip < 0).any() or (stop < 0).any():
        raise DecodeError(E_INVALID, int(np.flatnonzero(np.concatenate([skip, stop]) < 0)[0]))
    if row_stride == 0:
        o = np.asarray(tok_offsets, dtype=np.int64)
        n = len(o) - 1
        if o[0] < 0:
            raise DecodeError(E_INVALID, 0)
        if (np.diff(o) < 0).any():
            raise DecodeError(E_INVALID, int(np.flatnonzero(np.diff(o) < 0)[0]))
        if o[n] > len(ids):
            raise DecodeError(E_INVALID, n)
        seg_first, seg_n = o[:-1], np.diff(o)
    else:
        n = n_segs if lengths is None else len(lengths)
        if n * row_stride > len(ids):
            raise DecodeError(E_INVALID, -1)
        seg_n = np.full(n, row_stride, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
        if ((seg_n < 0) | (seg_n > row_stride)).any():
            raise DecodeError(E_INVALID, int(np.flatnonzero((seg_n < 0) | (seg_n > row_stride))[0]))
        seg_first = np.arange(n, dtype=np.int64) * row_stride
    seg = np.repeat(np.arange(n, dtype=np.int64), seg_n)
    seg_at = np.concatenate([[0], np.cumsum(seg_n)]).astype(np.int64)  # a segment's first entry among the repeated ones
    pos = seg_first[seg] + (np.arange(len(seg), dtype=np.int64) - seg_at[seg])
    v = ids[pos]
    stops = np.isin(v, stop)
    cum = np.cumsum(stops)
    before = cum - stops  # stop ids in front of an entry, over the whole call ...
    live = (before - before[seg_at[seg]] if len(seg) else before) == 0  # ... and since its segment began
    skipped = np.isin(v, skip) | (stops & (not keep_stop)) | ((v < 0) & bool(skip_negative))
    if skip_special:
        skipped |= np.isin(v, np.asarray(list(special_ids), dtype=np.int64))
    known = (v >= 0) & (v <= vocab.max_id)
    ln = np.where(known, vocab.lens[np.where(known, v, 0)], 0) if vocab.max_id >= 0 else np.zeros(len(v), dtype=np.int64)
    bad = live & ~skipped & (ln == 0)
    if bad.any():
        raise DecodeError(E_BAD_TOKEN, int(pos[bad].min()))
    emit = np.where(live & ~skipped, ln, 0)
    offs = np.concatenate([[0], np.cumsum(np.bincount(seg, weights=emit, minlength=n))]).astype(np.int64)
    seg_ids = np.bincount(seg, weights=live, minlength=n).astype(np.int64)
    sel = emit > 0
    src = np.repeat(vocab.begin[v[sel]], emit[sel]) + (np.arange(int(emit.sum())) - np.repeat(np.cumsum(emit[sel]) - emit[sel], emit[sel]))
    out = vocab.blob[src.astype(np.int64)].tobytes()
    info = np.asarray([len(out), sel.sum(), (live & ~sel).sum(), (live & stops).sum()], dtype=np.int64)
    return out, offs, seg_ids, info


def small_vocab(rng):
    """A vocabulary of 20 - 60 ids with holes (ids that are no token) and three special ids at its top -> (tok, special_ids)."""
    max_id = int(rng.integers(20, 60))
    tok = {}
    for i in range(max_id - 2):
        if rng.random() < 0.85:
            tok[i] = bytes(rng.integers(97, 123, size=int(rng.integers(1, 7))).astype(np.uint8))
    special = [max_id - 2, max_id - 1, max_id]
    for k, i in enumerate(special):
        tok[i] = b"<|s%d|>" % k
    return tok, special


def random_case(rng, max_segs=10, max_len=30, errors=True):
    """-> dict(tok, special_ids, ids, kw): kw are the keyword arguments of the truths.  Both forms; empty segments; stop ids (also
    first, also skipped as well) with ids behind them that are no tokens; negative ids; listed ids above max_id; rows of length 0 and
    row_stride; offsets that begin above 0 and end below n_tokens; with errors=True a tenth of the cases holds an id that is none."""
    tok, special = small_vocab(rng)
    max_id = max(tok)
    regular = [i for i in tok if i not in special]
    holes = [i for i in range(max_id + 1) if i not in tok] + [max_id + 7, 2**31 - 1]
    pad = max_id + 1 + int(rng.integers(0, 3))  # "models pad with n_vocab"
    skip_negative = bool(rng.random() < 0.5)
    skip_special = bool(rng.random() < 0.3)
    keep_stop = bool(rng.random() < 0.4)
    stop = [special[0]] if rng.random() < 0.8 else []
    if stop and rng.random() < 0.3:
        stop.append(int(rng.choice(regular)))
    if stop and rng.random() < 0.3:
        stop.append(pad + 5)  # a stop id above the vocabulary
    skip = [pad] if rng.random() < 0.7 else []
    if rng.random() < 0.4:
        skip += [special[1], int(rng.choice(regular))]
    if stop and rng.random() < 0.35:
        skip.append(stop[0])  # both skipped and stop
    if skip and rng.random() < 0.2:
        skip = skip + skip[:1]
    n_segs = int(rng.integers(0, max_segs + 1))
    rows = bool(rng.random() < 0.45)
    stride = int(rng.integers(1, max_len + 1)) if rows else 0
    lens = rng.integers(0, (stride if rows else max_len) + 1, size=n_segs)
    lens[rng.random(n_segs) < 0.2] = 0
    if rows:
        lens[rng.random(n_segs) < 0.2] = stride
    good = regular + special[1:] + skip + ([-100, -1] if skip_negative else [])
    if keep_stop:
        good = [x for x in good if not (x in stop and x not in tok and x not in skip)]  # (a kept stop id that is no token is an error)
    stop_ok = [x for x in stop if not keep_stop or x in tok or x in skip]
    segs = []
    for n in lens:
        s = [int(x) for x in rng.choice(good, size=int(n))] if n else []
        s = [x for x in s]
        if stop_ok and n and rng.random() < 0.6:
            at = 0 if rng.random() < 0.3 else int(rng.integers(0, n))
            s[at] = int(rng.choice(stop_ok))
            s[at + 1:] = [int(x) for x in rng.choice(holes + [-5, -100] + regular, size=int(n) - at - 1)]  # what a model leaves behind EOS
        segs.append(s)
    lead = int(rng.integers(1, 6)) if not rows and rng.random() < 0.4 else 0
    tail = int(rng.integers(1, 6)) if rng.random() < 0.4 else 0
    junk = lambda k: [int(x) for x in rng.choice(holes + [-7], size=k)]  # noqa: E731
    if rows:
        flat = []
        for s in segs:
            flat += s + junk(stride - len(s))
        kw = dict(row_stride=stride, lengths=lens.astype(np.int32), n_segs=n_segs)
        if n_segs and (lens == stride).all() and rng.random() < 0.5:
            kw["lengths"] = None
    else:
        flat = junk(lead) + [x for s in segs for x in s]
        kw = dict(tok_offsets=(lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64))
    flat += junk(tail)
    ids = np.asarray(flat, dtype=np.int64)
    if errors and len(ids) and rng.random() < 0.1:
        k = rng.integers(0, len(ids), size=2)
        ids[k] = rng.choice(holes + [-3], size=2)
    kw.update(skip=skip, stop=stop, keep_stop=keep_stop, skip_negative=skip_negative, skip_special=skip_special, special_ids=special)
    return dict(tok=tok, special_ids=special, ids=ids.astype(np.int32), kw=kw, pad=pad)
