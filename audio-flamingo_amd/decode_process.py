"""generate()'s built-in logits processors on the device - the processors GenerationMixin._get_logits_processor (transformers/generation/utils.py:1154-1290) puts
in front of the sampling warpers, applied in its order by one launch per step so that the decode step stays capturable (csrc/decode_process.hip; the contracts
are in include/afk.h):

   1. sequence_bias                          SequenceBiasLogitsProcessor
   2. repetition_penalty                     RepetitionPenaltyLogitsProcessor
   3. no_repeat_ngram_size                   NoRepeatNGramLogitsProcessor
   4. bad_words_ids                          NoBadWordsLogitsProcessor
   5. min_length                             MinLengthLogitsProcessor
   6. min_new_tokens                         MinNewTokensLengthLogitsProcessor
   7. forced_eos_token_id                    ForcedEOSTokenLogitsProcessor
   8. exponential_decay_length_penalty       ExponentialDecayLengthPenalty
   9. suppress_tokens, begin_suppress_tokens SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor

The launch is afk_decode_process while only 2, 3, 6 and 9 are active and afk_decode_process_ex as soon as one of 1, 4, 5, 7 or 8 is.

  resolve(...)      pure, CPU-runnable: merges the keywords with a generation config, validates as the reference does -> ProcessSpec
  pack_sequences(...)  pure: sequences with biases -> the packed table of afk_decode_process_ex, grouped by last id
  build_state(...)  the device state of a prompt batch: id history, seen-set bitmap, id lists, sequence tables, the decay table
  apply(...)        one launch on a [B, V] fp32 logits row block
  resolve_warpers(...)  pure, CPU-runnable: min_p / typical_p / epsilon_cutoff / eta_cutoff merged and validated the same way.  These four are no processors of
                    this file's launch: they sit behind top-p inside the sampler (afk_decode_sample_filtered, csrc/decode_sample.hip), where generate() sends them

Deliberately not covered (generate() keeps refusing them as keywords; in a generation config they stay ignored):
  * renormalize_logits - a row reduction behind the warpers, i.e. inside the sampler, not a processor of this launch;
  * remove_invalid_values - the reference itself documents that there is no use for it;
  * encoder_repetition_penalty / encoder_no_repeat_ngram_size - they read encoder input ids, which a decoder-only model does not have;
  * top_h - its warper sits in front of top-k inside the sampler and is a sequential scan;
  * prefix_allowed_tokens_fn - a host callback per step: pass it as logits_processor=[PrefixConstrainedLogitsProcessor(...)]."""
from __future__ import annotations

from typing import NamedTuple, Optional

NAMES = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens")
DEFAULTS = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, begin_suppress_tokens=None)
EX_NAMES = ("sequence_bias", "bad_words_ids", "min_length", "forced_eos_token_id", "exponential_decay_length_penalty")
EX_DEFAULTS = dict(sequence_bias=None, bad_words_ids=None, min_length=0, forced_eos_token_id=None, exponential_decay_length_penalty=None)


class ProcessSpec(NamedTuple):
    penalty: float = 1.0          # 1.0: off
    ngram: int = 0                # 0: off
    min_new_tokens: int = 0       # 0 whenever no EOS id is known: the ban has nothing to act on
    eos: tuple = ()               # the eos ids, kept only while min_new_tokens, min_length or decay needs them
    suppress: tuple = ()
    begin_suppress: tuple = ()
    sequence_bias: tuple = ()     # ((ids, bias), ...) in the reference dict's order
    bad_words: Optional[tuple] = None   # (ids, ...) in the reference dict's order, [eos] sequences filtered out; (): nothing left, the row still gets its + 0.0f
    min_length: int = 0           # 0 whenever no EOS id is known
    forced_eos: tuple = ()
    decay: tuple = ()             # (start, factor), or () = off

    @property
    def extended(self) -> bool:
        """one of the processors only afk_decode_process_ex applies is on"""
        return bool(self.sequence_bias or self.bad_words is not None or (self.min_length > 0 and self.eos) or self.forced_eos or self.decay)

    @property
    def active(self) -> bool:
        return bool(self.penalty != 1.0 or self.ngram > 0 or (self.min_new_tokens > 0 and self.eos) or self.suppress or self.begin_suppress or self.extended)


def _id_list(v, name):
    if v is None:
        return ()
    if hasattr(v, "tolist"):
        v = v.tolist()
    if isinstance(v, int) and not isinstance(v, bool):
        v = [v]
    if not isinstance(v, (list, tuple)) or any(isinstance(i, bool) or not isinstance(i, int) or i < 0 for i in v):
        raise ValueError(f"`{name}` has to be a list of positive integers, but is {v}")
    return tuple(int(i) for i in v)


def _is_id(i):
    import numpy as np

    return isinstance(i, (int, np.integer))


def _sequence_bias(sb):
    """SequenceBiasLogitsProcessor._validate_arguments with its messages, then its conversion of the list form -> ((ids, bias), ...) in dict order"""
    if not isinstance(sb, (dict, list)) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
    if isinstance(sb, dict):
        if any(not isinstance(ids, tuple) for ids in sb):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
        if any(len(ids) == 0 or any(not _is_id(i) or i < 0 for i in ids) for ids in sb):
            raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
        if any(not isinstance(b, float) for b in sb.values()):
            raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
    else:   # the list form refuses the id 0 (`token_id > 0`), as the reference does
        pair_ok = lambda q: (isinstance(q, (list, tuple)) and len(q) >= 2 and isinstance(q[0], list) and len(q[0]) > 0
                             and all(_is_id(i) and i > 0 for i in q[0]) and isinstance(q[1], float))
        if any(not pair_ok(q) for q in sb):
            raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {sb}.")
        sb = {tuple(q[0]): q[1] for q in sb}
    return tuple((tuple(int(i) for i in ids), float(b)) for ids, b in sb.items())


def _bad_words(bw, eos):
    """NoBadWordsLogitsProcessor.__init__: its validation and messages, the [eos] sequences filtered out, duplicates merged as its dict does -> (ids, ...)"""
    if not isinstance(bw, list) or len(bw) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
    if any(not isinstance(w, list) for w in bw):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
    if any(any(not _is_id(i) or i < 0 for i in w) for w in bw):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
    if any(len(w) == 0 for w in bw):   # the reference accepts it here and fails with an IndexError at the first step
        raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of positive integers, but is {bw}.")
    return tuple(dict.fromkeys(tuple(int(i) for i in w) for w in bw if all(list(w) != [e] for e in eos)))


def _eos_tensor_check(v):
    """the eos-list check of ForcedEOSTokenLogitsProcessor and ExponentialDecayLengthPenalty, with their message (it prints the tensor) -> the ids"""
    import torch

    t = v if isinstance(v, torch.Tensor) else torch.tensor([v] if isinstance(v, int) else v)
    if torch.is_floating_point(t) or bool((t < 0).any()):
        raise ValueError(f"`eos_token_id` has to be a list of positive integers, but is {t}")
    return tuple(int(i) for i in t.reshape(-1).tolist())


def resolve(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, begin_suppress_tokens=None, eos_token_id=None,
            generation_config=None, sequence_bias=None, bad_words_ids=None, min_length=0, forced_eos_token_id=None,
            exponential_decay_length_penalty=None) -> ProcessSpec:
    """keywords (+ a generation config for the ones left at their default, as GenerationMixin merges them; an explicit keyword wins) -> ProcessSpec.
    Validation is the reference's: the penalty must be a float > 0 (RepetitionPenaltyLogitsProcessor.__init__, its message), the n-gram size an int >= 0
    (0 = off; NoRepeatNGramLogitsProcessor refuses what is not a positive int), min_new_tokens an int >= 0 that only acts when an EOS id is known
    (utils.py:1227-1230); eos_token_id an int or a list of ints (taken from the config when the argument is None).  sequence_bias (the list-of-pairs form or
    the dict form) and bad_words_ids: the classes' _validate_arguments with their messages; bad words equal to [eos] are dropped.  min_length: an int >= 0
    (MinLengthLogitsProcessor.__init__, its message) that only acts when an EOS id is known (utils.py:1214-1218).  forced_eos_token_id: an int or a list with its
    class's check; it needs no eos_token_id.  exponential_decay_length_penalty = (start, factor): the class's check of the eos ids, and a ValueError when no EOS
    id is known (the reference fails there on torch.tensor(None))."""
    kw = dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens,
              begin_suppress_tokens=begin_suppress_tokens)
    ex = dict(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, min_length=min_length, forced_eos_token_id=forced_eos_token_id,
              exponential_decay_length_penalty=exponential_decay_length_penalty)
    gc = generation_config
    if gc is not None:
        for k in NAMES:
            if kw[k] == DEFAULTS[k] and getattr(gc, k, None) is not None:
                kw[k] = getattr(gc, k)
        for k in EX_NAMES:
            if ex[k] == EX_DEFAULTS[k] and getattr(gc, k, None) is not None:
                ex[k] = getattr(gc, k)
        if eos_token_id is None:
            eos_token_id = getattr(gc, "eos_token_id", None)
    for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens"):   # None = "unset" in a GenerationConfig
        if kw[k] is None:
            kw[k] = DEFAULTS[k]
    p = kw["repetition_penalty"]
    if p == 1 and not isinstance(p, bool):   # utils.py:1174 builds no processor for 1 / 1.0, so nothing validates it
        p = 1.0
    if not isinstance(p, float) or not (p > 0):
        raise ValueError(f"`penalty` has to be a strictly positive float, but is {p}")
    g = kw["no_repeat_ngram_size"]
    if isinstance(g, bool) or not isinstance(g, int) or g < 0:
        raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {g}")
    mn = kw["min_new_tokens"]
    if isinstance(mn, bool) or not isinstance(mn, int) or mn < 0:
        raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {mn}")
    decay = ex["exponential_decay_length_penalty"]
    if decay is not None:
        if eos_token_id is None:
            raise ValueError("`exponential_decay_length_penalty` needs an EOS id to act on: set `eos_token_id`")
        _eos_tensor_check(eos_token_id)
        if (not isinstance(decay, (tuple, list)) or len(decay) != 2 or isinstance(decay[0], bool) or not isinstance(decay[0], int)
                or isinstance(decay[1], bool) or not isinstance(decay[1], (int, float)) or not (decay[1] > 0)):
            raise ValueError(f"`exponential_decay_length_penalty` has to be a (start_index: int, decay_factor: float > 0) pair, but is {decay}")
        decay = (int(decay[0]), float(decay[1]))
    eos = _id_list(eos_token_id, "eos_token_id")
    ml = ex["min_length"]
    if ml is None:
        ml = 0
    if isinstance(ml, bool) or not isinstance(ml, int) or ml < 0:
        raise ValueError(f"`min_length` has to be a non-negative integer, but is {ml}")
    ml = int(ml) if eos else 0
    seq_bias = _sequence_bias(ex["sequence_bias"]) if ex["sequence_bias"] is not None else ()
    bad = _bad_words(ex["bad_words_ids"], eos) if ex["bad_words_ids"] is not None else None
    forced = _eos_tensor_check(ex["forced_eos_token_id"]) if ex["forced_eos_token_id"] is not None else ()
    return ProcessSpec(penalty=float(p), ngram=int(g), min_new_tokens=int(mn) if eos else 0, eos=eos if (mn > 0 or ml > 0 or decay) else (),
                       suppress=_id_list(kw["suppress_tokens"], "suppress_tokens"), begin_suppress=_id_list(kw["begin_suppress_tokens"], "begin_suppress_tokens"),
                       sequence_bias=seq_bias, bad_words=bad, min_length=ml, forced_eos=forced, decay=decay or ())


WARPER_DEFAULTS = dict(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
WARPERS_OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


def resolve_warpers(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, generation_config=None, do_sample=True) -> dict:
    """keywords (+ a generation config for the ones left at their default; an explicit keyword wins) -> the four values as ops.decode_sample takes them, an
    inactive filter at its "off" value.  As GenerationMixin._get_logits_processor gates them (utils.py:1323-1343): min_p whenever it is set, typical_p when
    < 1, epsilon_cutoff / eta_cutoff only inside (0, 1); the classes' own validation and wording (MinPLogitsWarper / TypicalLogitsWarper.__init__): min_p
    outside [0, 1] and typical_p <= 0 raise ValueError.  do_sample=False: nothing is built, so nothing is validated and all four are off."""
    kw = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
    gc = generation_config
    if gc is not None:
        for k in kw:
            if kw[k] == WARPER_DEFAULTS[k] and getattr(gc, k, None) is not None:
                kw[k] = getattr(gc, k)
    out = dict(WARPERS_OFF)
    if not do_sample:
        return out
    if kw["min_p"] is not None:
        if not (0 <= kw["min_p"] <= 1.0):
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {kw['min_p']}")
        out["min_p"] = float(kw["min_p"])
    if kw["typical_p"] is not None and kw["typical_p"] < 1.0:
        mass = float(kw["typical_p"])
        if not (mass > 0 and mass < 1):
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {mass}")
        out["typical_p"] = mass
    for k in ("epsilon_cutoff", "eta_cutoff"):
        if kw[k] is not None and 0.0 < kw[k] < 1.0:
            out[k] = float(kw[k])
    return out


def pack_sequences(seqs, V: int):
    """((ids, bias), ...) in the reference dict's order -> the packed table of afk_decode_process_ex as a dict of lists: the sequences grouped by their last id,
    groups in the order their id first occurs, the sequences of a group in the given order (a stable grouping: the fp32 sum of a group's biases keeps the
    reference's order).  group_id / group_l1 (the one-id sequence's bias, 0.0 without one) / group_off; per sequence of length >= 2 seq_bias and seq_off into
    ids, which holds the ids in front of the last one.  An id outside [0, V) is refused with SequenceBiasLogitsProcessor._prepare_bias_variables's message.
    No sequence at all (every bad word was an [eos]) packs to one group that adds 0.0f to id 0: the reference's processor still adds its zero bias to the row."""
    invalid = [i for ids, _ in seqs for i in ids if i >= V]
    if invalid:
        raise ValueError(f"The model vocabulary size is {V}, but the following tokens were being biased: {invalid}")
    groups = {} if seqs else {0: dict(l1=0.0, seqs=[])}
    for ids, bias in seqs:
        g = groups.setdefault(ids[-1], dict(l1=0.0, seqs=[]))
        if len(ids) == 1:
            g["l1"] = bias
        else:
            g["seqs"].append((ids[:-1], bias))
    tb = dict(ids=[], seq_off=[0], seq_bias=[], group_id=[], group_l1=[], group_off=[0])
    for last, g in groups.items():
        tb["group_id"].append(last), tb["group_l1"].append(g["l1"])
        for front, bias in g["seqs"]:
            tb["ids"].extend(front), tb["seq_off"].append(len(tb["ids"])), tb["seq_bias"].append(bias)
        tb["group_off"].append(len(tb["seq_bias"]))
    return tb


def _table_to(tb, dev):
    import torch

    f32 = ("seq_bias", "group_l1")   # a float list may hold infinities: through float64, which rounds to fp32 as torch.tensor(bias) does in the reference
    return {k: (torch.tensor(v, dtype=torch.float64).to(torch.float32) if k in f32 else torch.tensor(v, dtype=torch.int32)).to(dev) for k, v in tb.items()}


def decay_table(start: int, factor: float, max_new_tokens: int):
    """c[t] = float32(pow(factor, t - start) - 1) for t > start, 0 elsewhere (never read), in double on the host as ExponentialDecayLengthPenalty computes it"""
    import torch

    def c(t):
        try:
            return pow(factor, t - start) - 1
        except OverflowError:
            return float("inf")

    return torch.tensor([c(t) if t > start else 0.0 for t in range(int(max_new_tokens))], dtype=torch.float64).to(torch.float32)


def build_state(spec: ProcessSpec, ids, max_new_tokens: int, V: int):
    """device state of afk_decode_process / afk_decode_process_ex for the prompt batch ids [B, S0] (exactly what generate() was given: the reference's processors
    see padding and <sound> ids too): hist [B, S0 + max_new_tokens] int32 with the prompt in front, seen [B, ceil(V / 32)] int32 = the prompt's ids as a bitmap,
    the id lists; "ex" (only with one of the processors of afk_decode_process_ex on): the packed sequence tables, the forced ids and the decay table of
    max_new_tokens entries.  One-time setup in torch ops, outside the captured step."""
    import torch

    B, S0 = ids.shape
    dev = ids.device
    hist = torch.zeros((B, S0 + int(max_new_tokens)), device=dev, dtype=torch.int32)
    hist[:, :S0] = ids
    nwords = (V + 31) // 32
    mask = torch.zeros((B, nwords * 32), device=dev, dtype=torch.bool)
    rows, cols = torch.nonzero((ids >= 0) & (ids < V), as_tuple=True)   # an id outside the vocabulary marks nothing (the kernel skips it as well)
    mask[rows, ids[rows, cols].long()] = True
    weights = torch.tensor([1 << i for i in range(31)] + [-(1 << 31)], device=dev, dtype=torch.int64)   # bit 31 is the sign bit of the int32 word
    seen = (mask.view(B, nwords, 32).to(torch.int64) * weights).sum(-1).to(torch.int32).contiguous()
    lst = lambda t: torch.tensor(t, device=dev, dtype=torch.int32) if t else None
    ps = dict(spec=spec, S0=S0, hist=hist, seen=seen, suppress=lst(spec.suppress), begin_suppress=lst(spec.begin_suppress), eos=lst(spec.eos))
    if spec.extended:   # uploaded once: the sequence tables, the forced ids, one decay factor per token
        ps["ex"] = dict(bias=_table_to(pack_sequences(spec.sequence_bias, V), dev) if spec.sequence_bias else None,
                        bad=_table_to(pack_sequences(tuple((w, float("-inf")) for w in spec.bad_words), V), dev) if spec.bad_words is not None else None,
                        min_length=spec.min_length, forced_eos=lst(spec.forced_eos),
                        decay=decay_table(*spec.decay, max_new_tokens).to(dev) if spec.decay else None, decay_start=spec.decay[0] if spec.decay else 0,
                        max_new_tokens=int(max_new_tokens))
    return ps


def apply(ps, logits, *, next_token=None, step_base=None, step_off=0, **select_kw):
    """one launch on the fp32 logits [B, V] (in place) for token t = *step_base + step_off - afk_decode_process_ex when one of its processors is active,
    afk_decode_process otherwise; select_kw: ops.decode_process's selection block"""
    from . import ops

    spec = ps["spec"]
    kw = dict(S0=ps["S0"], penalty=spec.penalty, ngram=spec.ngram, suppress=ps["suppress"], begin_suppress=ps["begin_suppress"], eos=ps["eos"],
              min_new_tokens=spec.min_new_tokens, next_token=next_token, step_base=step_base, step_off=step_off, **select_kw)
    if "ex" in ps:
        return ops.decode_process_ex(logits, ps["hist"], ps["seen"], **ps["ex"], **kw)
    return ops.decode_process(logits, ps["hist"], ps["seen"], **kw)
