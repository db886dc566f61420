"""Plain-integer restatement of the contract of afk_decode_stop (include/afk.h) - EosTokenCriteria, StopStringCriteria.__call__ as a sequential recurrence over
the class's own table, the pad substitution and the stop_at / status bookkeeping - and tiny_tokenizer(), an in-memory byte-level tokenizer that puts chosen
strings at chosen ids so that stop strings can be built around the tokens a tiny random model happens to emit.  No download, no GPU."""
import numpy as np

INT_MAX = 2 ** 31 - 1


def table_of(criteria):
    """the run-time fields of a constructed StopStringCriteria as plain integers / numpy"""
    return dict(table=criteria.embedding_vec.cpu().numpy().astype(np.int64), P=int(criteria.max_valid_positions), E=int(criteria.max_valid_end_lens),
                S=int(criteria.num_stop_strings), target=[int(x) for x in criteria.target_lens.tolist()], W=int(criteria.maximum_token_len))


def string_match(ids, tab) -> bool:
    """ids: the row's n ids, oldest first -> does a stop string end at the last one (the rule of include/afk.h, step 3)"""
    if tab is None or tab["S"] == 0:
        return False
    T, P, E, S, W = tab["table"], tab["P"], tab["E"], tab["S"], tab["W"]
    rows, vec = T.shape
    assert vec == S * (P + E) + 1
    last = [min(int(i), rows - 1) if int(i) >= 0 else rows - 1 for i in list(ids)[-W:][::-1]]   # newest first, clamped to the dummy row
    for s in range(S):
        for e in range(E):
            c = int(T[last[0], P * S + E * s + e])
            if c <= 0:
                continue
            best = c
            for j in last[1:]:
                if not any(int(T[j, P * s + k]) == c for k in range(P)):
                    break
                c += int(T[j, vec - 1])
                best = max(best, c)
            if best >= tab["target"][s]:
                return True
    return False


def judge(ids, eos, tab) -> bool:
    return int(ids[-1]) in set(int(e) for e in eos) or string_match(ids, tab)


def step(next_token, ids, stop_at, status, t, *, S0, max_new, eos=(), pad=0, feed_pad=False, tab=None):
    """one launch of afk_decode_stop on numpy state, in place: next_token [B] int64, ids [B, ld] int32, stop_at [B] int32, status [2] int32"""
    if t < 0 or t >= max_new:
        return
    B = next_token.shape[0]
    for b in range(B):
        tok = int(next_token[b])
        if stop_at[b] < t:
            tok = pad
            if feed_pad:
                next_token[b] = pad
        ids[b, S0 + t] = tok
        if stop_at[b] >= t and judge(ids[b, : S0 + t + 1], eos, tab):
            stop_at[b] = t
    status[0] = t
    status[1] = int((stop_at > t).sum())


def _unicode_of(piece):
    from transformers.convert_slow_tokenizer import bytes_to_unicode

    m = bytes_to_unicode()
    return "".join(m[b] for b in (piece if isinstance(piece, (bytes, bytearray)) else piece.encode("utf-8")))


def tiny_tokenizer(pieces, vocab_size=1024):
    """PreTrainedTokenizerFast around an in-memory `tokenizers` byte-level BPE with no merges: pieces {id: str | bytes} sit at their ids (< vocab_size), the 256
    single-byte tokens at vocab_size .. vocab_size + 255 (a byte that a piece already is keeps its slot as a filler), and every other id holds a distinct filler
    piece made of control bytes only (0x00 .. 0x10), which no printable stop string touches."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    filler = lambda i: bytes([0]) + bytes(1 + int(d, 16) for d in f"{i:x}")
    vocab, taken = {}, set()
    for i, p in pieces.items():
        assert 0 <= i < vocab_size
        u = _unicode_of(p)
        assert u and u not in taken, f"piece {p!r} twice"
        taken.add(u)
    by_id = {i: _unicode_of(p) for i, p in pieces.items()}
    for b in range(256):
        u = _unicode_of(bytes([b]))
        if u not in taken:
            by_id[vocab_size + b] = u
            taken.add(u)
    for i in range(vocab_size + 256):
        vocab[by_id[i] if i in by_id else _unicode_of(filler(i))] = i
    assert len(vocab) == vocab_size + 256
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    tok.decoder = decoders.ByteLevel()
    return PreTrainedTokenizerFast(tokenizer_object=tok)
