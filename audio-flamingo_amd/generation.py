"""generate() of the MI355X-native Audio Flamingo 3 model: greedy decoding, sampling and beam search on the KV cache, host code only (docs/generate.md
tells the routes feature by feature; the forward pieces a step runs - _decode_logits, _decode_layers*, _chain_* - live in decode_forward.py).

  DecodeState        the record a decode step works on: the cache, the static device tensors, what the step applies
  _run_steps         the loop every route drives its step with: eager, captured at the second step, replayed, polled every eighth
  AfkGenerationMixin generate() and its routes, inherited by AudioFlamingo3ForConditionalGeneration"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, ops
from . import decode_assist as _assist
from . import decode_cfg as _cfg
from . import decode_lookup as _lookup
from . import decode_process as _process
from . import decode_share as _share
from . import decode_stop as _stop
from . import decode_w8 as _w8mod
from ._lib import AfkError


@dataclass
class SingleSequence:
    """one sequence: cur, position and the key-range end live in ONE device tensor, advanced by one add per step"""
    state: torch.Tensor     # int32 [4] = [lo, key-range end, cache slot, position]
    kr1: torch.Tensor       # state[0:2], the key range the attention reads
    pos1: torch.Tensor      # state[3:4], the rotary position
    advance: torch.Tensor   # state[1:4], what a step moves


@dataclass
class OnDevice:
    """one sequence with token selection and step bookkeeping on the device: the static buffers of that step"""
    x0: torch.Tensor                          # the embedding row of the token just selected: the next step's input
    tok_buf: torch.Tensor                     # int64 [max_new_tokens], the emitted tokens
    logits: Optional[torch.Tensor] = None     # fp32 [1, V]: sampled, processed or recorded steps
    part_val: Optional[torch.Tensor] = None   # plain greedy: the lm_head launch's (max, argmax) per eight rows
    part_idx: Optional[torch.Tensor] = None


@dataclass
class DecodeState:
    """what one decode step reads and writes; everything position-dependent is on the device, so the step can be captured.  A record: no behaviour."""
    cache: tuple            # (K, Vt) as AfkKVCache holds them
    lo: torch.Tensor        # int32 [B], first real position of every row
    head: torch.Tensor      # lm_head weight
    emb: torch.Tensor       # embed_tokens weight
    cur: torch.Tensor       # int32 [1], the cache slot the step appends at
    nxt: torch.Tensor       # int64 [B], the token just selected
    sampling: Optional[dict] = None   # the warpers and the seed (generate()); None: greedy
    proc: Optional[dict] = None       # decode_process.build_state
    rec: Optional[dict] = None        # {"logits", "scores"}: the [max_new_tokens, B, V] buffers of the output object
    stop: Optional[dict] = None       # decode_stop.build_state
    aws: Optional[torch.Tensor] = None   # workspace of the Q = 1 attention (allocated by the first step that needs it)
    tok_off: Optional[int] = None     # token number = *cur + tok_off
    single: Optional[SingleSequence] = None
    on_device: Optional[OnDevice] = None
    shared: Optional[_share.SharedPrompt] = None   # the prompt cache of a call that shares it (decode_share.py): `cache` is then the TAIL cache, cur counts its slots from 0
    w8: Optional[_w8mod.DecodeW8] = None   # FP8 decode weights (decode_w8.py): the single-sequence chain - with decode_weights_batched the 2 - 8-row chain too - streams this copy of its Linears and of the lm_head
    cfg: Optional[_cfg.CfgState] = None   # classifier-free guidance (decode_cfg.py): cache, lo and nxt have 2 * B rows - [0, B) conditional, [B, 2B) unconditional - and everything else B


def _run_steps(step, max_new, use_graph, closed, after=None):
    """steps 1 .. max_new - 1 of a decode loop (token 0 is the caller's) -> the number of steps run.  Step 1 runs eagerly (lazy one-time initialisation
    inside the library happens outside the capture); with use_graph (None: whenever more than 3 tokens are asked for) step 2 is captured into a HIP graph
    and replayed from then on.  closed(t) is asked in front of every 8th step, and the loop ends when it says so.  after(): host work behind every
    step, outside the capture."""
    if use_graph is None:
        use_graph = max_new > 3
    graph, n = None, 0
    for t in range(1, max_new):
        if t % 8 == 0 and closed(t):
            break
        if use_graph and t == 2:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            graph.replay()  # capture only records: the step for t == 2 itself still has to run
        elif graph is not None:
            graph.replay()
        else:
            step()
        if after is not None:
            after()
        n += 1
    return n


def continuation_lengths(P, S_total, who="generate(past_key_values=...)"):
    """generate() on a passed cache: input_ids is the WHOLE conversation and the cache covers its first P positions (GenerationMixin._prefill,
    transformers/generation/utils.py:3918-3938: "the `input_ids` are ... the FULL sequence, including previous inputs"; it slices
    input_ids[:, -(S_total - P):] and has no check of its own for P >= S_total).  -> P; ValueError naming both numbers when nothing is left to run"""
    P, S_total = int(P), int(S_total)
    if P >= S_total:
        raise ValueError(f"{who}: the cache already holds {P} positions and input_ids has {S_total}; input_ids must be the whole conversation, at least "
                         f"one token longer than the cache")
    return P


def continuation_mask_check(attention_mask, lo, P, S_total, who="generate(past_key_values=...)"):
    """the attention_mask of a continuation covers all S_total positions: its first P columns must be the left padding the cache records (zeros in front
    of lo[b], ones from there) and the suffix all ones.  Anything else would be a hole in the keys a row sees, which the key-interval kernels cannot
    express.  Pure: CPU or device tensors."""
    if attention_mask.dim() != 2 or attention_mask.shape[0] != lo.shape[0] or attention_mask.shape[1] != int(S_total):
        raise AfkError(f"{who}: attention_mask {tuple(attention_mask.shape)} must cover the whole conversation [{lo.shape[0]}, {int(S_total)}] (cache of "
                       f"{int(P)} positions + the new ones)")
    want = torch.arange(int(S_total), device=attention_mask.device)[None, :] >= lo.to(attention_mask.device)[:, None].long()
    if not bool((attention_mask.bool() == want).all()):
        raise AfkError(f"{who}: attention masks with holes are not supported - the first {int(P)} columns must repeat the left padding of the cache "
                       f"(first real positions {lo.tolist()}) and the new positions must all be real")


class AfkGenerationMixin:
    beam_on_device = os.environ.get("AFK_BEAM_DEVICE", "1") == "1"   # beam search: the step's decisions and the cache move as launches of the decode step (csrc/decode_beam.hip)
    lookup_on_device = os.environ.get("AFK_LOOKUP_DEVICE", "1") == "1"   # prompt-lookup decoding: the draft and accept rules as launches of the step (csrc/decode_lookup.hip); off: torch ops and host reads
    assist_on_device = os.environ.get("AFK_ASSIST_DEVICE", "1") == "1"   # assisted decoding: the draft model's steps and the two rules around them as launches of one step (csrc/decode_assist.hip); off: torch ops and host reads
    last_assist_stats = None   # the last generate() call with an assistant_model: {emitted, steps, accepted, rejecting, launched, drafted}; None after every other call
    share_prompt_cache = os.environ.get("AFK_SHARE_PROMPT", "0") == "1"   # generate(share_prompt=None): sampled copies and device beams share the prompt's keys (decode_share.py, csrc/attention_shared.hip)
    last_share_stats = None   # the last generate() call that shared a prompt cache: decode_share.stats; None after every other call
    last_cfg_stats = None   # the last generate() call under classifier-free guidance: decode_cfg.stats; None after every other call

    # ------------------------------------------------------------------ the pieces of a step
    @staticmethod
    def _select_token(logits, sampling=None):
        """greedy argmax, or GenerationMixin's sampling chain on the [B, V] fp32 logits of the new position: temperature -> top-k -> top-p
        (TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper, transformers/generation/logits_process.py) -> softmax -> multinomial.
        Token selection is O(B*V) index work outside the training hot path: plain torch ops."""
        if not sampling:
            return logits.argmax(-1)
        t, k, p_, gen = sampling["temperature"], sampling["top_k"], sampling["top_p"], sampling["generator"]
        if t and t != 1.0:
            logits = logits / t
        if k and k > 0:
            kth = logits.topk(min(k, logits.shape[-1]), -1).values[..., -1:]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        if p_ is not None and p_ < 1.0:
            sl, si = logits.sort(-1, descending=False)
            drop = sl.softmax(-1).cumsum(-1) <= (1.0 - p_)
            drop[..., -1:] = False  # always keep the most likely token
            logits = logits.masked_fill(drop.scatter(-1, si, drop), float("-inf"))
        return torch.multinomial(logits.softmax(-1), 1, generator=gen).squeeze(-1)

    @staticmethod
    def _record_rows(rec, which, rows, *, step_base=None, step_off=0):
        """generate(output_logits / output_scores): one afk_decode_record launch that keeps the fp32 rows [B, V] in slot *step_base + step_off of rec[which]
        ([max_new_tokens, B, V]).  Nothing is enqueued when the buffer was not asked for, or when `scores` shares the buffer of `logits` (greedy decoding with
        no processor: the row is recorded once, under "logits")."""
        if not rec or rec.get(which) is None or (which == "scores" and rec.get("logits") is rec["scores"]):
            return
        if rows.dtype != torch.float32 or rows.stride(-1) != 1:   # only what a user logits_processor returned (token 0 and the eager hook loop): the captured
            rows = rows.float().contiguous()                      # steps hand over the fp32 rows the lm_head wrote, so nothing is allocated or copied there
        ops.decode_record(rows, rec[which], step_base=step_base, step_off=step_off)

    @staticmethod
    def _scores_kw(rec):
        """the sampler's keywords that make its launch keep the warped row (afk_decode_sample_scored); {} when scores were not asked for"""
        return dict(scores_out=rec["scores"]) if rec and rec.get("scores") is not None else {}

    @staticmethod
    def _sample_token(logits, sampling, **kw):
        """the sampling chain of _select_token on the device, in one launch and with no host state (ops.decode_sample): temperature -> top-k -> top-p ->
        min_p -> typical_p -> epsilon_cutoff -> eta_cutoff -> the draw from a counter-based generator keyed by sampling["seed"]; kw: the draw's counter
        (step_base / step_off) and the outputs.  Every sampled token of generate() - the first, the batched step, the one-sequence chain, the hook loop - comes
        through here with the same `sampling` dict."""
        if logits.dtype != torch.float32 or logits.stride(-1) != 1:
            logits = logits.float().contiguous()
        return ops.decode_sample(logits, temperature=sampling["temperature"], top_k=sampling["top_k"], top_p=sampling["top_p"], seed=sampling["seed"],
                                 min_p=sampling["min_p"], typical_p=sampling["typical_p"], epsilon_cutoff=sampling["epsilon_cutoff"],
                                 eta_cutoff=sampling["eta_cutoff"], **kw)

    @staticmethod
    def _guided_rows(st, logits):
        """the rows of a step's logits the selection works on, their unconditional partners and the tokens' place in st.nxt: everything as it is without
        guidance; under it (st.cfg) logits is [2 * B, V] and the three are views - rows [0, B), rows [B, 2B), nxt[:B].  Host code only."""
        if st.cfg is None:
            return logits, None, st.nxt
        B = st.cfg.B
        return logits[:B], logits[B:], st.nxt[:B]

    def _record_and_process(self, st, logits, *, step_base=None, step_off=0, uncond=None, **select):
        """the front of every route's token: the raw row recorded in front of the processors, then the built-in processors in place (`select`: the launch
        also selects greedily from the row it leaves and does the step's bookkeeping, ops.decode_process).  uncond (classifier-free guidance: the unconditional
        rows of the same step): between the two, afk_decode_cfg folds each pair into the conditional row, in place - stage 0 of the processor list, behind the
        record, so `logits` keeps the raw conditional rows as the reference's raw_logits does"""
        self._record_rows(st.rec, "logits", logits, step_base=step_base, step_off=step_off)
        if uncond is not None:
            ops.decode_cfg(logits, uncond, st.cfg.scale, out=logits, ws=st.cfg.ws)
        if st.proc:   # the token being generated is number cur + 1 - S0: the processors' (and the draw's) counter lives on the device and advances with the step
            _process.apply(st.proc, logits, next_token=st.nxt if st.cfg is None else st.nxt[:st.cfg.B], step_base=step_base, step_off=step_off, **select)

    def _pick_token(self, st, logits, *, step_base=None, step_off=0, record=True, out=None, **book):
        """the token of the processed rows, into `out` where given: the draw (whose launch keeps the warped row where scores were asked for; book: the
        bookkeeping it does for a single sequence), or the row recorded as the step's score and its argmax"""
        if st.sampling:
            return self._sample_token(logits, st.sampling, step_base=step_base, step_off=step_off, out=out, **book, **self._scores_kw(st.rec))
        if record:
            self._record_rows(st.rec, "scores", logits, step_base=step_base, step_off=step_off)
        tok = self._select_token(logits)
        return tok if out is None else out.copy_(tok)

    def _select_on_device(self, st, x):
        """the tail of the single-sequence step whose selection stays on the device, behind the layers' residual row x: the lm_head launch, then ONE launch
        for argmax or the draw / the token / the positions / the next embedding row"""
        od, rec, off = st.on_device, st.rec, st.tok_off
        book = dict(tokens_out=od.tok_buf, tok_off=off, state=st.single.state, emb=st.emb, x_out=od.x0)
        if st.sampling or st.proc:
            # sampled, or logits processors: the lm_head launch writes the fp32 logits; the processors' launch edits the row (and, greedy, selects from it and
            # does the bookkeeping); the sample launch draws and does the bookkeeping
            self._chain_lm_head(x, st.head, logits=od.logits, w8=st.w8)
            select = {} if st.sampling else dict(select=True, **book)   # greedy: st.proc is set here
            self._record_and_process(st, od.logits, step_base=st.cur, step_off=off, **select)
            if select:
                # the selecting launch has advanced state[2] (= cur) itself, and the processed row it selected from is still in place: recorded BEHIND it,
                # one step further back (rather than inside the launch, which would put a vocabulary-sized store into afk_decode_process for this case only)
                self._record_rows(rec, "scores", od.logits, step_base=st.cur, step_off=off - 1)
            else:
                self._pick_token(st, od.logits, step_base=st.cur, step_off=off, out=st.nxt, **book)
            return
        # plain greedy: the lm_head launch leaves (max, argmax) per eight rows, the select launch does everything up to the next step.  Flags off: no logits
        # row is written; on: the same launch also leaves the row (the partial argmax pairs, hence the ids, are the same)
        self._chain_lm_head(x, st.head, logits=od.logits if rec else None, part_val=od.part_val, part_idx=od.part_idx, w8=st.w8)
        if rec:   # no processor: scores and logits are the same rows (one buffer when both are asked for); in front of the select launch, which advances cur
            self._record_rows(rec, "logits", od.logits, step_base=st.cur, step_off=off)
            self._record_rows(rec, "scores", od.logits, step_base=st.cur, step_off=off)
        _lib.call("afk_decode_select_greedy", od.part_val.data_ptr(), od.part_idx.data_ptr(), od.part_val.numel(), st.nxt.data_ptr(), od.tok_buf.data_ptr(), off,
                  st.single.state.data_ptr(), st.emb.data_ptr(), st.emb.stride(0), st.emb.shape[1], od.x0.data_ptr(), ops._stream())

    def _decode_step(self, st):
        """one greedy or sampled decode step on static buffers (everything position-dependent lives on the device): HIP-graph capturable"""
        if st.on_device is not None:   # one sequence: 5 launches per layer + lm_head + ONE launch for argmax or the draw / token / positions / the next embedding row
            x = self._chain_layers(st.on_device.x0, st.cache, st.single.pos1, st.single.kr1, st.cur, aws=st.aws, w8=st.w8)
            self._select_on_device(st, x)
            if st.stop:   # behind the selection launch, which has advanced cur (= state[2]) already: one step back.  The next embedding row is in x0: no pad is fed
                _stop.apply(st.stop, st.nxt, step_base=st.cur, step_off=st.tok_off - 1)
            return
        logits, uncond, nxt = self._guided_rows(st, self._decode_logits(st))
        self._record_and_process(st, logits, step_base=st.cur, step_off=st.tok_off, uncond=uncond)
        self._pick_token(st, logits, step_base=st.cur, step_off=st.tok_off, out=nxt)
        if st.stop:   # the stopping rule on the token just selected; a row that finished earlier emits pad_token_id and the next step embeds it
            _stop.apply(st.stop, nxt, step_base=st.cur, step_off=st.tok_off, feed_pad=True)
        if uncond is not None:   # the unconditional row of a pair is fed the token of its conditional row (pad behind the row's end): one small copy
            st.nxt[st.cfg.B:].copy_(nxt)
        (st.single.advance if st.single is not None else st.cur).add_(1)   # single sequence: cur, position and the key-range end live in one tensor

    def _new_state(self, cache, lo, cur, nxt, **kw):
        return DecodeState(cache=cache, lo=lo, head=self.arena["lm_head.weight"].data, emb=self.arena[self._lm + "embed_tokens.weight"].data,
                           cur=torch.full((1,), cur, device=self.device_, dtype=torch.int32), nxt=nxt, **kw)

    # ------------------------------------------------------------------ beam search
    @torch.no_grad()
    def _beam_search(self, ids, last_hidden, cache, lo, nb, max_new, eos, pad, length_penalty, early_stopping, *, num_return=1, use_graph=None, share=None, w8=None):
        """Beam search on the KV cache with GenerationMixin's scoring (transformers/generation/utils.py:3008-3400): every batch row keeps `nb`
        running beams ranked by accumulated log-probability; at each step the best (n_eos + 1) * nb continuations over all beams are drawn, the
        ones among the top nb that end (EOS, or the length limit) compete for the row's nb FINISHED slots with score = sum / generated_length ^
        length_penalty, the best nb that do not end continue.  The loop stops when no running beam can still beat the worst finished one
        (the reference's heuristic: best running sum / current generated length ^ length_penalty; early_stopping = True: as soon as every
        finished slot is filled; "never": the optimistic bound at the maximum length when length_penalty > 0) or the length limit is reached.
        The KV cache is reordered by beam parentage every step.  eos: the ids as a tuple, pad: the id behind a hypothesis's end (decode_stop.resolve).
        Returns the best num_return finished hypotheses per row as [B * num_return, S0 + longest], padded with pad.
        Two routes with identical results: _beam_search_device (beam_on_device, inside the caps of afk_beam_step, AFK_EXACT_FP32 off), otherwise the
        host loop below: torch ops over [B, nb * V], one host synchronisation and one index_select copy of the whole cache per token."""
        from . import exact as _exact

        dev = self.device_
        B, S0 = ids.shape
        V = self.V
        if share is not None:   # the prompt cache is the prefill's own (no headroom, no per-beam copy); the beams' generated positions live in a tail cache
            shared, tail, lo_rep, rep = self._share_setup(share, cache, lo, S0, max_new)
            return self._beam_search_device(ids, last_hidden, tail, lo_rep, rep, nb, max_new, eos, pad, length_penalty, early_stopping, num_return, use_graph, shared=shared, w8=w8)
        rep = torch.arange(B, device=dev).repeat_interleave(nb)   # one cache row per beam
        Kc, Vt = cache[0].index_select(1, rep).contiguous(), cache[1].index_select(1, rep).contiguous()
        lo = lo.index_select(0, rep).contiguous()
        if self.beam_on_device and not _exact.ENABLED and ops.beam_caps_ok(nb, len(eos), V):
            return self._beam_search_device(ids, last_hidden, (Kc, Vt), lo, rep, nb, max_new, eos, pad, length_penalty, early_stopping, num_return, use_graph, w8=w8)
        keep = (len(eos) + 1) * nb
        st = self._new_state((Kc, Vt), lo, S0, torch.zeros(B * nb, device=dev, dtype=torch.int64), w8=w8)
        run_seq = torch.zeros((B, nb, max_new), device=dev, dtype=torch.int64)
        run_score = torch.full((B, nb), -1.0e9, device=dev, dtype=torch.float32)
        run_score[:, 0] = 0.0                                           # all beams of a row start identical: only the first one is live
        fin_seq = torch.zeros((B, nb, max_new), device=dev, dtype=torch.int64)
        fin_len = torch.zeros((B, nb), device=dev, dtype=torch.int64)
        fin_score = torch.full((B, nb), -1.0e9, device=dev, dtype=torch.float32)
        fin_done = torch.zeros((B, nb), device=dev, dtype=torch.bool)
        logits = ops.gemm_nt(last_hidden, st.head).float().index_select(0, rep)      # next-token logits after the prompt, one copy per beam
        top_mask = torch.arange(keep, device=dev) < nb
        boff = (torch.arange(B, device=dev) * nb)[:, None]
        can_improve = torch.ones((B, 1), device=dev, dtype=torch.bool)
        for t in range(max_new):
            logp = torch.log_softmax(logits, dim=-1).view(B, nb, V) + run_score[:, :, None]
            cand_score, cand = logp.view(B, nb * V).topk(keep, dim=-1)
            parent, tok = cand // V, cand % V
            cand_seq = run_seq.gather(1, parent[:, :, None].expand(B, keep, max_new)).clone()
            cand_seq[:, :, t] = tok
            ends = torch.zeros_like(tok, dtype=torch.bool)
            for e in eos:
                ends |= tok == e
            if t + 1 == max_new:
                ends[:] = True                                            # the length limit finishes whatever is left
            # finished slots: candidates among the top nb that end, scored sum / generated_length ^ length_penalty
            fscore = cand_score / float((t + 1) ** length_penalty)
            full = fin_done.all(-1, keepdim=True) & (early_stopping is True)
            fscore = fscore + (full | ~can_improve | ~(ends & top_mask[None])).float() * -1.0e9
            ms, mi = torch.cat([fin_score, fscore], 1).topk(nb, dim=-1)
            fin_seq = torch.cat([fin_seq, cand_seq], 1).gather(1, mi[:, :, None].expand(B, nb, max_new))
            fin_len = torch.cat([fin_len, torch.full_like(tok, t + 1)], 1).gather(1, mi)
            fin_done = torch.cat([fin_done, ends & top_mask[None]], 1).gather(1, mi)
            fin_score = ms
            # running beams: the best nb candidates that do not end
            rs, ri = (cand_score + ends.float() * -1.0e9).topk(nb, dim=-1)
            run_seq, run_score = cand_seq.gather(1, ri[:, :, None].expand(B, nb, max_new)), rs
            if t + 1 == max_new:
                break
            # can a running beam still beat the worst finished hypothesis?  (reference heuristic, utils.py:3008-3052)
            hyp_len = (max_new if (early_stopping == "never" and length_penalty > 0.0) else (t + 1))
            best_running = run_score[:, :1] / float(hyp_len ** length_penalty)
            worst_fin = torch.where(fin_done, fin_score.min(-1, keepdim=True).values, torch.full_like(fin_score, -1.0e9))
            can_improve = can_improve & (best_running > worst_fin).any(-1, keepdim=True)
            if not bool(can_improve.any()) or (early_stopping is True and bool(fin_done.all())):
                break
            # advance the model: reorder the cache by parentage, feed the chosen tokens
            src = (parent.gather(1, ri) + boff).reshape(-1)
            Kc.copy_(Kc.index_select(1, src)), Vt.copy_(Vt.index_select(1, src))
            st.nxt.copy_(tok.gather(1, ri).reshape(-1))
            logits = self._decode_logits(st)
            st.cur.add_(1)
        return self._beam_result(ids, fin_seq, fin_len, num_return, pad)

    @staticmethod
    def _beam_result(ids, fin_seq, fin_len, n, pad):
        """the best n finished hypotheses of every row (fin_seq [B, nb, max_new], fin_len [B, nb], in ranking order) behind the prompt: [B * n, S0 + longest],
        row b * n + k = hypothesis k of row b, padded with pad (0 where neither a pad nor an eos id is known) - the reference's order and shape"""
        B, _, max_new = fin_seq.shape
        best_seq, best_len = fin_seq[:, :n].reshape(B * n, max_new), fin_len[:, :n].reshape(B * n)
        best_seq = torch.where(torch.arange(max_new, device=best_seq.device)[None] < best_len[:, None], best_seq, torch.full_like(best_seq, pad if pad is not None else 0))
        return torch.cat([ids.repeat_interleave(n, dim=0) if n > 1 else ids, best_seq[:, : int(best_len.max())]], dim=1)

    @torch.no_grad()
    def _beam_search_device(self, ids, last_hidden, cache, lo, rep, nb, max_new, eos, pad, length_penalty, early_stopping, num_return, use_graph, shared=None, w8=None):
        """_beam_search with every per-token decision on the device (cache, lo: one row per beam, rep: each one's prompt row).  A step is _decode_logits -> afk_beam_step (log-softmax, the row's top (n_eos + 1) * nb
        continuations, finished slots, running beams, the early-stop heuristic, {t, open} in a status word) -> afk_beam_reorder_cache (the slots written since
        the prompt move by parentage, in place: the beams of a row share their prompt keys bit for bit) -> cur += 1; nothing in it depends on the host, so it is
        captured and replayed (_run_steps).  Token 0 runs eagerly with the kernel of the captured steps.  The host polls the status word every 8th step (steps
        behind the closing one write nothing) and reads the finished hypotheses back once.
        shared (generate(share_prompt=True)): `cache` is the tail cache and the prompt keys stay in the prefill's own cache, one row per prompt row - the
        slots count from 0, so the reorder moves the slots 0 .. cur of the tail and no prompt key is ever copied."""
        B, S0 = ids.shape
        Kc, Vt = cache
        bs = ops.beam_state(B, nb, max_new, device=self.device_, eos=eos, length_penalty=length_penalty, early_stopping=early_stopping)
        if shared is not None:
            S0 = 0   # of the cache the step appends to
        st = self._new_state(cache, lo, S0, bs["next_token"], shared=shared, w8=w8)
        ops.beam_step(ops.gemm_nt(last_hidden, st.head).float().index_select(0, rep).contiguous(), bs, step_off=0)

        def step():   # token t = cur + 1 - S0: the forward pass appends the keys of token t - 1 at slot cur, so the slots S0 .. cur move
            logits = self._decode_logits(st)
            ops.beam_step(logits if logits.is_contiguous() else logits.contiguous(), bs, step_base=st.cur, step_off=1 - S0)
            ops.beam_reorder_cache(Kc, Vt, bs["src"], st.cur, nb=nb, S0=S0, max_new=max_new)
            st.cur.add_(1)

        _run_steps(step, max_new, use_graph, lambda t: bs["status"].tolist()[1] == 0)   # one small copy, {last step, open}
        fin_seq, fin_len, _, _ = ops.beam_finished(bs)
        return self._beam_result(ids, fin_seq, fin_len, num_return, pad)

    # ------------------------------------------------------------------ generate
    @torch.no_grad()
    def generate(self, input_ids, input_features=None, input_features_mask=None, attention_mask=None, max_new_tokens=20,
                 do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=None, eos_token_id=None, pad_token_id=None, use_cache=True,
                 use_graph=None, num_beams=1, length_penalty=1.0, early_stopping=False, generation_config=None, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, begin_suppress_tokens=None, min_p=None, typical_p=1.0,
                 epsilon_cutoff=0.0, eta_cutoff=0.0, num_return_sequences=None, sequence_bias=None, bad_words_ids=None, min_length=0,
                 forced_eos_token_id=None, exponential_decay_length_penalty=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=None, share_prompt=None,
                 guidance_scale=None, negative_prompt_ids=None, negative_prompt_attention_mask=None, decode_weights=None, assistant_model=None,
                 num_assistant_tokens=None, decode_weights_batched=None, **kwargs):
        """Greedy decoding, sampling or beam search on a KV cache, with GenerationMixin.generate's arguments and results; docs/generate.md describes every
        route, what it launches and how it differs from the reference.

        input_ids [B, S0], input_features / input_features_mask (audio, merged in the prefill), attention_mask (LEFT padding only).
        max_new_tokens (20, > 0).  use_cache (True; False: the greedy recompute path of the tests).  use_graph (None: capture the decode step into a HIP
        graph whenever more than 3 tokens are asked for).
        do_sample (False) with temperature (1.0) / top_k (50; 1 is greedy) / top_p (1.0) / min_p / typical_p (1.0) / epsilon_cutoff (0.0) / eta_cutoff (0.0)
        and seed (None: from torch.seed()): one seed gives the same ids on every route.
        num_beams (1) with length_penalty (1.0) / early_stopping (False, True, "never"); num_return_sequences (1; needs beams or do_sample).
        sequence_bias / repetition_penalty (1.0) / no_repeat_ngram_size (0) / bad_words_ids / min_length (0) / min_new_tokens (0) / forced_eos_token_id /
        exponential_decay_length_penalty / suppress_tokens / begin_suppress_tokens: the built-in logits processors, applied in this order (the reference's) by
        one launch per token, in front of logits_processor= and the warpers.  Not built: renormalize_logits, remove_invalid_values, encoder_*, top_h,
        prefix_allowed_tokens_fn (decode_process.py says why).
        eos_token_id (int, list, tuple or tensor) / pad_token_id (default: the first eos id) / stop_strings= with tokenizer=.
        logits_processor= / stopping_criteria= / streamer=: the reference's per-step hooks; with one of them the steps run eagerly.
        return_dict_in_generate= with output_scores= / output_logits=: an AfkGenerateOutput (sequences, scores, logits, past_key_values) in place of the ids.
        prompt_lookup_num_tokens (k) with max_matching_ngram_size (2): prompt-lookup decoding - a step drafts up to k tokens by n-gram lookup in the ids so far,
        verifies them in one pass over the weights and emits the confirmed ones plus one; the ids are the plain greedy ids.  Greedy, one sequence, KV cache.
        past_key_values (None): continue on a cache - the AfkKVCache a previous generate(return_dict_in_generate=True) or forward(use_cache=True) returned, or the
        reference's DynamicCache.  The reference's semantics (GenerationMixin._prefill, transformers/generation/utils.py:3918-3938: input_ids is the FULL
        sequence and is sliced to the positions the cache does not hold; _prepare_cache_for_generation :1946-1958 takes a user cache as it is;
        prepare_inputs_for_generation :552 slices, :616 forwards the multimodal inputs on the first forward of a continuation; AF3 overrides none of them):
        input_ids [B, S_total] is the whole conversation, the cache covers its first P positions, the model runs on ids[:, P:] (n rows behind a long past: the
        split-KV append attention, afk_attn_append), input_features are the audio of the <sound> ids inside that suffix only, attention_mask covers S_total
        (the cache's left padding, then ones).  The cache is updated in place - it holds every token but the last - and is the output object's
        past_key_values.  Greedy or sampled decoding with everything below; docs/generate.md, "Continuing from a cache".
        share_prompt (None: the class attribute share_prompt_cache, env AFK_SHARE_PROMPT, default off): the sampled copies (do_sample with
        num_return_sequences = n) or the device beams of a row share ONE prefill and ONE copy of the prompt's keys; a step attends to the prompt cache and
        a short tail cache of generated positions (afk_attn_decode_shared).  False, or nothing to share: not one launch or allocation differs.  The ids can
        differ from the unshared call on near-ties (the prefill runs on other row counts); docs/generate.md, "Sharing the prompt".
        guidance_scale (None; keyword, else the generation config) with negative_prompt_ids [B, Sn] (None: the last id of every prompt row) and
        negative_prompt_attention_mask (LEFT padding): classifier-free guidance, the reference's UnbatchedClassifierFreeGuidanceLogitsProcessor - active for
        any scale but None and 1 (inactive: the negative prompt is ignored, and not one launch or allocation differs).  Every prompt row gets an unconditional
        row (the negative prompt, text only, its own cache rows, the same selected tokens) in the same decode step - one pass over the weights for both -
        and afk_decode_cfg replaces the row's logits by scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond) in front of every
        processor; `logits` keeps the raw conditional rows, past_key_values the conditional cache.  docs/generate.md, "Classifier-free guidance".
        decode_weights (None: the class attribute decode_weight_dtype, env AFK_DECODE_WEIGHTS, default "bf16"): "fp8" - the decode steps of ONE sequence stream
        an FP8 copy of the decoder Linears and the lm_head (OCP e4m3fn codes, one power-of-two scale per output row: half the bytes; decode_w8.py), built on
        first use and rebuilt when the weights have changed.  Weights only: the prefill, the activations and the cache are what they are, and the decode logits
        differ from the bf16 route by the quantisation.  "bf16": not one launch or allocation differs.  docs/generate.md, "FP8 decode weights".
        decode_weights_batched (None: the class attribute decode_weights_batched, env AFK_DECODE_WEIGHTS_BATCHED, default off) with decode_weights "fp8": decode
        steps of 2 - 8 rows - a batch of prompts, num_return_sequences copies, beams, an active guidance_scale, the verify pass of prompt-lookup decoding,
        share_prompt=True - read the same FP8 copy through the matrix-pipe launches of the batched chain (afk_decode_chain_*_batched_w8).  Off: not one launch,
        allocation, refusal or result differs; one row decodes as decode_weights alone says.  docs/generate.md, "FP8 decode weights, 2 - 8 rows".
        assistant_model (None) with num_assistant_tokens (k; None: the assistant's generation_config.num_assistant_tokens, else 5): assisted (speculative)
        decoding - a second, smaller model of this package with the same vocabulary drafts k tokens per step on a cache of its own (prefilled with the same
        prompt and audio), this model verifies them in one pass over its weights and emits the confirmed ones plus one; the ids are the plain greedy ids.  The
        whole step - the k draft steps included - is launches only (afk_assist_begin / afk_assist_stage around the single-sequence chain, then the verify
        forward and afk_lookup_accept) and is captured like every other route; the class attribute assist_on_device (env AFK_ASSIST_DEVICE, default on) off,
        or a draft geometry outside the single-sequence chain: the same rules as torch ops with host reads, eagerly.  Greedy, one sequence, a fresh bf16 KV
        cache; every step drafts exactly k tokens (num_assistant_tokens_schedule "constant") and assistant_confidence_threshold is ignored.  None: not one
        launch or allocation differs.  last_assist_stats; docs/generate.md, "Assisted decoding".
        generation_config (default: self.generation_config if there is one) supplies every argument left at its default.

        Returns the ids [B * num_return_sequences, S0 + n]: the prompt, then the new tokens, pad_token_id behind a row's end.

        Raises ValueError where the reference's validation does (max_new_tokens <= 0, num_return_sequences, min_p / typical_p, eos / pad / stop_strings
        forms, stop strings without a tokenizer, prompt-lookup values <= 0 or a batch) and AfkError for what is not built: prompt-lookup decoding with anything
        but plain greedy decoding of one sequence (decode_lookup.resolve); an assistant_model of another class, device or vocabulary, with more than 31 drafted
        tokens, or with anything but plain greedy decoding of one sequence on a fresh bf16 cache (decode_assist.resolve; num_assistant_tokens <= 0 or no integer
        and a batch: ValueError); unknown keywords, synced_gpus / use_model_defaults;
        attention masks that are not left padding; beams with do_sample or use_cache=False; the logits processors, hooks, stop strings or the output
        object with beams or with use_cache=False; stop strings or the output object with AFK_EXACT_FP32=1; tokenizer= without a stop string;
        output_attentions / output_hidden_states; past_key_values with num_beams > 1, use_cache=False, AFK_EXACT_FP32=1 or num_return_sequences > 1, with an
        attention mask that has holes (AfkError), or with a cache that is not shorter than input_ids (ValueError naming both lengths); share_prompt=True
        with use_cache=False, AFK_EXACT_FP32=1, past_key_values, the per-step hooks, prompt-lookup decoding, the host beam loop or a geometry outside the
        batched decode chain (decode_share.resolve); guidance_scale with num_beams > 1, use_cache=False, AFK_EXACT_FP32=1, prompt-lookup decoding,
        past_key_values or share_prompt=True, with a negative prompt that holds the audio id or a negative mask that is not left padding (AfkError), with
        negative_prompt_ids of another batch size or a mask of another shape (ValueError) (decode_cfg.resolve); decode_weights="fp8" with more than one
        row, num_beams > 1, num_return_sequences > 1, guidance_scale, prompt-lookup decoding, share_prompt=True, use_cache=False, AFK_EXACT_FP32=1 or a
        geometry the single-sequence chain or its FP8 launches do not take (AfkError), any other value (ValueError); with decode_weights_batched: more than
        8 rows in a decode step, assistant_model=, use_cache=False, AFK_EXACT_FP32=1 or a step outside the norm-in-prologue launches (AfkError)
        (decode_w8.resolve)."""
        self._require_hip()
        self.last_share_stats = self.last_cfg_stats = self.last_w8_stats = self.last_assist_stats = None
        procs, criteria, streamer = kwargs.pop("logits_processor", None), kwargs.pop("stopping_criteria", None), kwargs.pop("streamer", None)
        out_kw = {k: kwargs.pop(k, None) for k in ("return_dict_in_generate", "output_scores", "output_logits", "output_attentions", "output_hidden_states")}
        stop_strings, tokenizer = kwargs.pop("stop_strings", None), kwargs.pop("tokenizer", None) or None
        past = kwargs.pop("past_key_values", None)   # None: a fresh prefill, and not one launch or allocation differs
        for k in ("synced_gpus", "use_model_defaults"):
            if kwargs.get(k):
                raise AfkError(f"generate({k}=...) is not supported by this implementation")
            kwargs.pop(k, None)
        if kwargs:
            raise AfkError(f"generate(): unknown / unsupported arguments {sorted(kwargs)}")
        hooks = bool(procs) or bool(criteria) or streamer is not None   # GenerationMixin's per-step callbacks: host code between the steps -> eager steps
        gc = generation_config if generation_config is not None else getattr(self, "generation_config", None)
        if gc is not None:  # explicit arguments win; anything still at its default is taken from the generation config
            pick = lambda cur, default, name: getattr(gc, name, None) if (cur == default and getattr(gc, name, None) is not None) else cur
            max_new_tokens = pick(max_new_tokens, 20, "max_new_tokens")
            do_sample, temperature, top_k, top_p = pick(do_sample, False, "do_sample"), pick(temperature, 1.0, "temperature"), pick(top_k, 50, "top_k"), pick(top_p, 1.0, "top_p")
            num_beams, length_penalty, early_stopping = pick(num_beams, 1, "num_beams"), pick(length_penalty, 1.0, "length_penalty"), pick(early_stopping, False, "early_stopping")
            eos_token_id, pad_token_id = pick(eos_token_id, None, "eos_token_id"), pick(pad_token_id, None, "pad_token_id")
        # the ten built-in logits processors: keyword, else generation config, validated as the reference does
        spec = _process.resolve(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, begin_suppress_tokens, eos_token_id=eos_token_id,
                                generation_config=gc, sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, min_length=min_length,
                                forced_eos_token_id=forced_eos_token_id, exponential_decay_length_penalty=exponential_decay_length_penalty)
        from . import exact as _exact
        from . import generation_output as _gout

        # the stopping rule: the eos ids as a tuple, pad defaulted to the first of them, stop strings (keyword, else generation config) with their refusals.
        # Every route below takes eos and pad in this form
        stop_spec = _stop.resolve(eos_token_id, pad_token_id, stop_strings, tokenizer, generation_config=gc, num_beams=int(num_beams), use_cache=bool(use_cache),
                                  exact_fp32=_exact.ENABLED)
        eos, pad = stop_spec.eos, stop_spec.pad
        n_ret = _gout.resolve_num_return_sequences(num_return_sequences, generation_config=gc, num_beams=int(num_beams), do_sample=bool(do_sample))
        flags = _gout.resolve_output_flags(**out_kw, generation_config=gc, num_beams=int(num_beams), use_cache=bool(use_cache), exact_fp32=_exact.ENABLED)
        if past is not None:
            bad = [what for what, on in (("num_beams > 1", int(num_beams) > 1), ("use_cache=False", not use_cache), ("AFK_EXACT_FP32=1", _exact.ENABLED),
                                         ("num_return_sequences > 1", n_ret > 1)) if on]
            if bad:
                raise AfkError(f"generate(past_key_values=...) with {' / '.join(bad)}: a passed cache continues greedy or sampled decoding of its own rows on "
                               f"the KV cache only")
        if int(max_new_tokens) <= 0:   # GenerationMixin refuses it as well (generation/configuration_utils.py validate())
            raise ValueError(f"`max_new_tokens` must be greater than 0, but is {max_new_tokens}.")
        # classifier-free guidance: keyword, else generation config, with every refusal; None: inactive (no scale, or 1), and nothing below changes
        cfg = _cfg.resolve(guidance_scale, negative_prompt_ids, negative_prompt_attention_mask, gc, batch_size=input_ids.shape[0],
                           audio_token_id=getattr(self, "audio_token_id", None), num_beams=int(num_beams), use_cache=bool(use_cache), exact_fp32=_exact.ENABLED,
                           lookup=prompt_lookup_num_tokens is not None or getattr(gc, "prompt_lookup_num_tokens", None) is not None, past=past is not None,
                           share_prompt=share_prompt, assist=assistant_model is not None)
        if cfg is not None and share_prompt is None:
            share_prompt = False   # the class attribute on: a guided call takes the unshared route, silently
        # prompt-lookup decoding: keyword, else generation config; None: off, and nothing below changes
        lookup = _lookup.resolve(prompt_lookup_num_tokens, max_matching_ngram_size, gc, batch_size=input_ids.shape[0], do_sample=bool(do_sample), num_beams=int(num_beams),
                                 use_cache=bool(use_cache), exact_fp32=_exact.ENABLED, processors=spec.active or bool(procs), hooks=bool(criteria) or streamer is not None,
                                 stop_strings=bool(stop_spec.stop_strings), output_object=flags.return_dict)
        # assisted decoding: the keyword; None: off, and nothing below changes
        assist = None
        if assistant_model is not None:
            assist = self._assist_resolve(assistant_model, num_assistant_tokens, batch_size=input_ids.shape[0], do_sample=bool(do_sample), num_beams=int(num_beams),
                                          copies=n_ret, use_cache=bool(use_cache), exact_fp32=_exact.ENABLED, processors=spec.active or bool(procs),
                                          hooks=bool(criteria) or streamer is not None, stop_strings=bool(stop_spec.stop_strings), output_object=flags.return_dict,
                                          past=past is not None, share_prompt=share_prompt, guidance=cfg is not None, decode_weights=decode_weights,
                                          lookup=lookup is not None, prompt_len=input_ids.shape[1], max_new_tokens=max_new_tokens)
        # the shared prompt cache: keyword, else the class attribute; None: off or nothing to share, and nothing below changes
        share = self._share_resolve(share_prompt, input_ids.shape[0], n_ret, int(num_beams), bool(use_cache), _exact.ENABLED, past is not None, hooks, lookup is not None, len(eos),
                                    assist=assist is not None)
        # FP8 decode weights: keyword, else the class attribute; False: today's route, and nothing below changes
        fp8 = self._w8_resolve(decode_weights, input_ids.shape[0] * (n_ret if int(num_beams) == 1 else 1), int(num_beams), n_ret, cfg is not None, lookup is not None,
                               share_prompt, bool(use_cache), _exact.ENABLED, assist=assist is not None, batched=decode_weights_batched,
                               lookup_rows=lookup.k + 1 if lookup is not None else None)
        if spec.active and (num_beams > 1 or not use_cache):
            raise AfkError("generate(repetition_penalty / no_repeat_ngram_size / min_new_tokens / suppress_tokens / begin_suppress_tokens / sequence_bias / "
                           "bad_words_ids / min_length / forced_eos_token_id / exponential_decay_length_penalty): greedy or sampled decoding on the KV cache "
                           "only (no num_beams > 1, no use_cache=False)")
        if _exact.ENABLED and not do_sample and num_beams == 1 and not hooks and not spec.active and type(self).__name__ == "AudioFlamingo3ForConditionalGeneration":
            # AFK_EXACT_FP32=1: greedy decoding by exact-fp32 recomputation of the prefix (exact.py) - the reference's greedy ids with no "confident rows" filter
            return _exact.greedy_generate(self, input_ids, input_features, input_features_mask, attention_mask, max_new_tokens, list(eos) or None, pad)
        if num_beams > 1 and (do_sample or not use_cache):
            raise AfkError("generate(num_beams > 1): beam search is deterministic and runs on the KV cache (no do_sample, no use_cache=False)")
        if hooks and (num_beams > 1 or not use_cache):
            raise AfkError("generate(logits_processor / stopping_criteria / streamer): greedy or sampled decoding on the KV cache only")
        sampling = None
        warp = _process.resolve_warpers(min_p, typical_p, epsilon_cutoff, eta_cutoff, generation_config=gc, do_sample=bool(do_sample) and num_beams == 1)
        if do_sample and int(top_k or 0) != 1:   # top_k == 1 is greedy selection (and keeps the no-logits path)
            sampling = dict(temperature=float(temperature) if temperature else 1.0, top_k=int(top_k or 0), top_p=1.0 if top_p is None else float(top_p),
                            seed=(int(seed) if seed is not None else int(torch.seed())) & (2 ** 64 - 1), **warp)
        ids = input_ids.to(self.device_)
        if n_ret > 1 and int(num_beams) == 1 and share is None:   # sampled copies: GenerationMixin._expand_inputs_for_generation - every tensor input repeated row by row; the
            expand = lambda x: x.repeat_interleave(n_ret, dim=0) if torch.is_tensor(x) else x   # draw is keyed by (step, row), so the copies differ
            ids, input_features, input_features_mask, attention_mask = expand(ids), expand(input_features), expand(input_features_mask), expand(attention_mask)
            if cfg is not None:   # the negative prompt and its mask like the other inputs
                cfg = cfg._replace(negative_ids=expand(cfg.negative_ids), negative_mask=expand(cfg.negative_mask))
        if not use_cache:
            if do_sample:
                raise AfkError("generate(use_cache=False) is the greedy reference path of the tests")
            return self._generate_recompute(ids, input_features, input_features_mask, attention_mask, max_new_tokens, eos)
        B, S0 = ids.shape
        dev = self.device_
        max_new = int(max_new_tokens)
        # a lookup step writes the cache slots of all its k + 1 rows; only the accepted ones ever become visible, so the cache needs k more positions
        headroom = max_new_tokens + (lookup.k if lookup else 0) + (assist.k if assist else 0)   # (an assisted step: the same k + 1 rows)
        if share is not None or cfg is not None:   # the prompt rows run once, into a cache that only ever holds the prompt: the generated positions go to the tail
            headroom = 0                           # cache (sharing) or to the combined cache of both branches (guidance)
        cont = self._continue_from(past, attention_mask, B, S0, headroom) if past is not None else None   # (the caller's object, its AfkKVCache form, P)
        if cont is not None and cont[1] is not None:
            # a passed cache: only the suffix ids[:, P:] runs - its <sound> rows take the audio of THIS call - as n new rows behind P cached positions, on the
            # split-KV append attention; from `last` on the call is the one below, with S0 the whole conversation
            kv, P = cont[1], cont[2]
            lo, Kc, Vt, pos_rows, krange = self._continue_setup(kv, attention_mask, B, S0, headroom, "generate(past_key_values=...)")
            x = self._merged_embeddings(ids[:, P:].contiguous(), input_features, input_features_mask)
            y = self._decode_layers(x, B, S0 - P, P, (Kc, Vt), pos_rows, krange, False, append=True)
            last = y.reshape(B, S0 - P, -1)[:, -1, :].contiguous()
        else:
            lo, padded, Kc, Vt, pos_rows, krange, fast = self._prefill_setup(attention_mask, B, S0, headroom, "generate()")
            x = self._merged_embeddings(ids, input_features, input_features_mask)
            y = self._decode_layers(x, B, S0, 0, (Kc, Vt), pos_rows, krange, fast, kv_lo=lo if padded else None)
            last = y.reshape(B, S0, -1)[:, -1, :].contiguous()
            if cont is not None:   # an EMPTY reference cache: the fresh prefill above (the LDS causal kernels, left padding included), written back at the end
                from .modeling import AfkKVCache

                cont = (cont[0], AfkKVCache(Kc, Vt, lo, 0), 0)
        if num_beams > 1:
            return self._beam_search(ids, last, (Kc, Vt), lo, int(num_beams), max_new, eos, pad, float(length_penalty), early_stopping, num_return=n_ret, use_graph=use_graph, share=share,
                                     w8=self._w8_current() if fp8 else None)
        first_logits = ops.gemm_nt(last, self.arena["lm_head.weight"].data).float()
        V = first_logits.shape[1]
        shared = None
        if share is not None:
            # sampled copies on a shared prompt: the B prompt rows were prefilled once; from here on the call has B * n rows - the first logits and the id
            # history the processors and the stop rule keep are repeated row by row, the cache the steps append to is the tail cache, slots from 0
            shared, (Kc, Vt), lo, rep = self._share_setup(share, (Kc, Vt), lo, S0, max_new)
            first_logits, ids, B = first_logits.index_select(0, rep).contiguous(), ids.index_select(0, rep).contiguous(), B * share.n
        guide = uncond_first = None
        if cfg is not None:
            # classifier-free guidance: the unconditional rows are prefilled on their own (text only, their own length) and both prompts move into ONE cache of
            # 2 * B rows, aligned to the right at slot Smax; from here on lo has 2 * B entries and the steps append at Smax, Smax + 1, ...
            guide, (Kc, Vt), lo, uncond_first = self._cfg_setup(cfg, ids, (Kc, Vt), lo, S0, max_new, V)
        if lookup is not None:
            return self._continue_done(cont, self._generate_lookup(ids, first_logits, (Kc, Vt), lo, lookup, max_new, eos, use_graph,
                                                                  w8=self._w8_current() if fp8 else None))
        if assist is not None:
            return self._generate_assisted(ids, input_features, input_features_mask, attention_mask, first_logits, (Kc, Vt), lo, assist, max_new, eos, use_graph)
        rec = None
        if flags.collect:   # one [max_new_tokens, B, V] fp32 buffer per kind, allocated once: static memory the captured step writes a slot of
            new_buf = lambda: torch.empty((max_new, B, V), device=dev, dtype=torch.float32)
            rec = {"logits": new_buf() if flags.logits else None, "scores": None}
            if flags.scores:   # greedy with no processor of any kind: the reference returns the same tensors in both tuples - one buffer, one record per step
                rec["scores"] = rec["logits"] if (flags.logits and not sampling and not spec.active and not procs and guide is None) else new_buf()
            self._record_rows(rec, "logits", first_logits, step_off=0)   # token 0, eagerly, with the kernel of the captured steps
        if guide is not None:   # token 0, eagerly, with the kernel of the captured steps: behind the record of the raw row, in front of every processor
            ops.decode_cfg(first_logits, uncond_first, guide.scale, out=first_logits, ws=guide.ws)
        proc = None
        if spec.active:   # token 0, eagerly, with the kernel of the captured steps; in front of the user's processors (GenerationMixin._merge_criteria_processor_list)
            proc = _process.build_state(spec, ids, max_new, V)
            _process.apply(proc, first_logits)
        if procs:
            first_logits = procs(ids, first_logits)
        if not sampling:
            self._record_rows(rec, "scores", first_logits, step_off=0)
        tok0 = self._sample_token(first_logits, sampling, **self._scores_kw(rec)) if sampling else self._select_token(first_logits)
        cur0 = S0 if shared is None else 0   # the cache slot the first step appends at; the token it selects is number cur + tok_off
        if guide is not None:   # both rows of a pair are fed the token; the slots count from where both prompts end
            tok0, cur0 = torch.cat([tok0, tok0]), guide.Smax
        st = self._new_state((Kc, Vt), lo, cur0, tok0, sampling=sampling, tok_off=1 - cur0, proc=proc, rec=rec, shared=shared, cfg=guide)   # the first token is draw 0
        if fp8:   # the copy of the weights as they are now (built or rebuilt here, outside every capture); the steps below read it through st.w8
            st.w8 = self._w8_current()
        sel = (lambda: st.nxt) if guide is None else (lambda: st.nxt[:B])   # the tokens of the B selected rows
        stop = None
        if stop_spec.device:   # more than one eos id, or stop strings: the rule is a launch of the step.  Token 0, eagerly, with the kernel of the captured steps
            stop = st.stop = _stop.build_state(stop_spec, ids, max_new, _stop.build_table(tokenizer, stop_spec.stop_strings) if stop_spec.stop_strings else None)
            _stop.apply(stop, sel(), step_off=0)
        if B == 1 and guide is None:   # (guidance: two cache rows, the batched route) one device tensor [lo, key-range end, cache slot, position] -> the views the kernels read; one add per step moves the last three
            state = torch.cat([lo, torch.tensor([S0 + 1, S0], device=dev, dtype=torch.int32), S0 - lo]).contiguous()
            st.cur, st.single = state[2:3], SingleSequence(state=state, kr1=state[0:2], pos1=state[3:4], advance=state[1:4])
            if not hooks and self._chain_ok(1) and V % 8 == 0:   # token selection (argmax or the draw) and step bookkeeping stay on the device
                tok_buf = torch.zeros(max_new_tokens, device=dev, dtype=torch.int64)
                tok_buf[0] = st.nxt[0]
                st.on_device = od = OnDevice(x0=st.emb.index_select(0, st.nxt).contiguous(), tok_buf=tok_buf)
                st.aws = self._decode_attn_workspace(dev, Vt.shape[4])
                if sampling or proc or rec:
                    od.logits = torch.empty((1, V), device=dev, dtype=torch.float32)
                if not (sampling or proc):   # plain greedy: the lm_head launch leaves partial (max, argmax) pairs
                    od.part_val, od.part_idx = torch.empty(V // 8, device=dev, dtype=torch.float32), torch.empty(V // 8, device=dev, dtype=torch.int32)
        if hooks:
            seq = self._generate_with_hooks(ids, st, first_logits, max_new, procs, criteria, streamer, eos, pad)
            return self._continue_done(cont, self._generate_output(flags, seq, S0, rec, st.cache, lo, cfg=guide))
        od = st.on_device
        toks = [sel().clone()]
        eos1 = eos[0] if eos else None   # the scalar route (one eos id, no stop string): token buffers compared on the host, no stop launch
        if stop is not None:
            closed = lambda t: stop["status"].tolist()[1] == 0   # the poll keeps its cadence: one small copy, {last step, rows still open}
        else:
            closed = lambda t: eos1 is not None and bool(((od.tok_buf[None, :t] if od is not None else torch.stack(toks, 1)) == eos1).any(1).all())
        n_new = 1 + _run_steps(lambda: self._decode_step(st), max_new, use_graph, closed, after=None if od is not None else lambda: toks.append(sel().clone()))
        if stop is not None:   # the reference's shape and padding: up to the step at which the last row finished; later steps only touched slots beyond it
            n_new = min(n_new, min(int(stop["stop_at"].max()), max_new) + 1)
            new = stop["ids"][:, S0:S0 + n_new].to(torch.int64)
        else:
            new = od.tok_buf[None, :n_new].clone() if od is not None else torch.stack(toks, 1)
            if eos1 is not None:  # everything after a row's first EOS becomes padding (GenerationMixin semantics)
                after = (new == eos1).cumsum(1) - (new == eos1).long() > 0
                new = torch.where(after, torch.full_like(new, pad), new)
        return self._continue_done(cont, self._generate_output(flags, torch.cat([ids, new], dim=1), S0, rec, st.cache, lo, shared=shared, cfg=guide))

    def _share_resolve(self, share_prompt, B0, copies, num_beams, use_cache, exact_fp32, past, hooks, lookup, n_eos, assist=False):
        """decode_share.resolve with what only the model knows: whether the device beam step takes the call, whether B0 * n rows take the batched decode chain
        and the geometry lies inside afk_attn_decode_shared's envelope"""
        n = num_beams if num_beams > 1 else copies
        on = self.share_prompt_cache if share_prompt is None else share_prompt
        geometry = beam_device = True
        if on and n > 1:   # asked only where the answer is read: with the switch off the call reads no weight and no attribute it did not read before
            geometry = ops.attn_shared_supported(self.Hq, self.Hkv, self.D, n) and self._chain_batched_ok(B0 * n, self.arena["lm_head.weight"].data)
            beam_device = self.beam_on_device and ops.beam_caps_ok(num_beams, n_eos, self.V)
        return _share.resolve(share_prompt, self.share_prompt_cache, copies=copies, num_beams=num_beams, use_cache=use_cache, exact_fp32=exact_fp32, past=past,
                              hooks=hooks, lookup=lookup, beam_device=beam_device, geometry=geometry, assist=assist)

    def _assist_resolve(self, assistant_model, num_assistant_tokens, **flags):
        """decode_assist.resolve with what only the two models know: the assistant's class and device, both vocabularies, both position limits"""
        from .modeling import AudioFlamingo3ForConditionalGeneration

        is_model = isinstance(assistant_model, AudioFlamingo3ForConditionalGeneration)   # Music Flamingo's class derives from it
        vocab = lambda m: (m.arena[m._lm + "embed_tokens.weight"].data.shape[0], m.arena["lm_head.weight"].data.shape[0], m.audio_token_id)
        limits = (int(self.config.text_config.max_position_embeddings), int(assistant_model.config.text_config.max_position_embeddings)) if is_model else None
        return _assist.resolve(assistant_model, num_assistant_tokens, is_model=is_model, same_device=not is_model or assistant_model.arena["lm_head.weight"].data.device == self.arena["lm_head.weight"].data.device,
                               target_vocab=vocab(self) if is_model else None, assistant_vocab=vocab(assistant_model) if is_model else None, max_positions=limits, **flags)

    def _cfg_setup(self, cfg, ids, cond_cache, lo, S0, max_new, V):
        """the unconditional branch of a guided call behind the main prefill (UnbatchedClassifierFreeGuidanceLogitsProcessor.get_unconditional_logits'
        first pass, logits_process.py:2294-2312): its prompt is cfg.negative_ids [B, Sn] - None: the last id of every prompt row - with no audio, prefilled by
        the ordinary set-up into a cache of its own; then decode_cfg.build lays both prompts into the combined cache, and the call's last_cfg_stats
        -> (CfgState, the combined cache, lo [2 * B], the unconditional first logits [B, V] fp32)"""
        B = ids.shape[0]
        neg = cfg.negative_ids.to(self.device_) if cfg.negative_ids is not None else ids[:, -1:].contiguous()
        Sn = neg.shape[1]
        lo_u, padded, Ku, Vu, pos_rows, krange, fast = self._prefill_setup(cfg.negative_mask, B, Sn, 0, "generate(negative_prompt_attention_mask=...)")
        y = self._decode_layers(self._merged_embeddings(neg, None, None), B, Sn, 0, (Ku, Vu), pos_rows, krange, fast, kv_lo=lo_u if padded else None)
        uncond_first = ops.gemm_nt(y.reshape(B, Sn, -1)[:, -1, :].contiguous(), self.arena["lm_head.weight"].data).float()
        guide, cache, lo2 = _cfg.build(cfg.scale, cond_cache, lo, S0, (Ku, Vu), lo_u, Sn, max_new, V)
        self.last_cfg_stats = _cfg.stats(guide, cache)
        return guide, cache, lo2, uncond_first

    def _share_setup(self, share, prompt_cache, lo, S0, max_new):
        """decode_share.build behind the prefill, and the call's last_share_stats -> (SharedPrompt, the tail cache, lo per continuation, rep)"""
        shared, tail, lo_rep, rep = _share.build(share, prompt_cache, lo, S0, max_new, self.Hq, self.Hkv, self.D)
        self.last_share_stats = _share.stats(shared, tail, max_new)
        return shared, tail, lo_rep, rep

    def _continue_from(self, past, attention_mask, B, S_total, headroom):
        """generate(past_key_values=past) -> (the caller's object, the AfkKVCache the call works on, P).  An AfkKVCache is worked on directly; the reference's
        DynamicCache is adopted into one (AfkKVCache.adopt, as forward(past_key_values=...) adopts it) and written back at the end; an EMPTY DynamicCache
        gives (past, None, 0): generate() runs its ordinary fresh prefill and writes the whole cache back."""
        from .modeling import AfkKVCache

        if isinstance(past, AfkKVCache):
            return past, past, continuation_lengths(past.length, S_total)
        if not AfkKVCache.is_reference_cache(past):
            raise AfkError("generate(past_key_values=...): pass the AfkKVCache a previous generate(return_dict_in_generate=True) or forward(use_cache=True) returned, "
                           "or the reference's DynamicCache")
        P = continuation_lengths(past.get_seq_length(), S_total) if int(past.get_seq_length()) else 0
        kv = AfkKVCache.adopt(past, self.dec_layers, self.Hkv, self.D, S_total - P, headroom, self.device_, attention_mask)
        return past, kv, P   # kv None: the cache is empty

    def _continue_done(self, cont, result):
        """the end of a call on a passed cache: the AfkKVCache holds every token but the last (its K / Vt were replaced by _continue_setup if it grew), a
        reference cache receives the positions [P, that length), and the output object carries the caller's own object"""
        if cont is None:
            return result
        past, kv, P = cont
        seq = result if torch.is_tensor(result) else result.sequences
        kv.length = int(seq.shape[1]) - 1
        if past is not kv:
            kv.write_back(past, P, kv.length - P, self.Hkv, self.D)
        if not torch.is_tensor(result):
            result.past_key_values = past
        return result

    @torch.no_grad()
    def _generate_lookup(self, ids, first_logits, cache, lo, lookup, max_new, eos, use_graph, w8=None):
        """greedy decoding of one sequence by prompt lookup (decode_lookup.py): token 0 is the argmax of the prefill's logits; from then on a step is
        afk_lookup_draft (up to k candidates from the ids so far + the k + 1 input rows) -> _lookup_forward (one pass over the weights, the rows appended at the
        cache slots cur .. cur + k) -> afk_lookup_accept (row argmaxes, the confirmed prefix + one token, ids / tokens / status / [end, cur, position] advanced by
        the number emitted).  Nothing in it depends on the host, so _run_steps captures and replays it; the host polls the status words every 8th step (steps
        behind `done` change nothing) and reads the emitted tokens back once.  lookup_on_device = False: the two rules in torch ops with host reads around the
        same forward, eagerly - the same ids and counters.  self.last_lookup_stats: {emitted, steps, accepted, rejecting} of the call and `launched`, the steps
        enqueued (the device route learns of the end at its next poll: up to seven more than `steps`)."""
        dev, S0, M = self.device_, ids.shape[1], lookup.k + 1
        if S0 + max_new + lookup.k > int(self.config.text_config.max_position_embeddings):
            raise AfkError(f"generate(prompt_lookup_num_tokens={lookup.k}): prompt {S0} + max_new_tokens {max_new} + {lookup.k} drafted positions exceed "
                           f"max_position_embeddings {int(self.config.text_config.max_position_embeddings)}")
        head, emb = self.arena["lm_head.weight"].data, self.arena[self._lm + "embed_tokens.weight"].data
        state = torch.cat([lo, torch.tensor([S0 + 1, S0], device=dev, dtype=torch.int32), S0 - lo]).contiguous()   # [lo, key-range end, cache slot, position]
        ls = _lookup.build_state(lookup, ids, self._select_token(first_logits), max_new, eos, state, emb.shape[1])
        aws = self._decode_attn_workspace(dev, cache[1].shape[4], M) if self._lookup_chain_ok(M, head) else None
        on_device = self.lookup_on_device
        draft, accept = (_lookup.draft, _lookup.accept) if on_device else (_lookup.draft_host, _lookup.accept_host)

        def step():
            draft(ls, emb)
            accept(ls, self._lookup_forward(ls["x"], cache, ls["pos"], ls["krange"], state[2:3], aws, head, w8=w8))

        done = lambda t=0: ls["status"].tolist()[_lookup.DONE] != 0   # one small copy
        launched = 0
        if on_device:
            launched = _run_steps(step, max_new, use_graph, done)
        else:
            while not done():
                step()
                launched += 1
        st = ls["status"].tolist()
        self.last_lookup_stats = dict(emitted=st[_lookup.EMITTED], steps=st[_lookup.STEPS], accepted=st[_lookup.ACCEPTED], rejecting=st[_lookup.REJECTING],
                                      launched=launched)
        return torch.cat([ids, ls["tokens"][None, :st[_lookup.EMITTED]]], dim=1)

    @torch.no_grad()
    def _generate_assisted(self, ids, input_features, input_features_mask, attention_mask, first_logits, cache, lo, assist, max_new, eos, use_graph):
        """greedy decoding of one sequence with a draft model (decode_assist.py): the assistant is prefilled on the same ids, audio and mask through its own
        audio tower into a cache of its own (k + 1 positions of headroom), so slots and positions agree between the two models; token 0 is the argmax of the
        target's prefill logits; from then on a step is
          afk_assist_begin (the assistant's step state <- the target's, its input row <- its embedding of the last emitted token)
          -> k single-sequence steps of the assistant (_chain_layers -> _chain_lm_head, partial argmaxes only -> afk_decode_select_greedy: draft token j, its
             input's keys at slot cur + j) -> ONE more _chain_layers pass on the last draft (its keys at slot cur + k: when all k drafts are accepted the next
             step starts behind it, and without it the assistant would attend to a hole there - the ids would stay right and the acceptance rate drop)
          -> afk_assist_stage (the drafts as candidates, cut behind an eos id and to the budget + the target's k + 1 input rows)
          -> _lookup_forward (one pass over the target's weights) -> afk_lookup_accept (the confirmed prefix + one token; [end, cur, position] advanced).
        The next step's begin copies the advanced state, which rewinds the assistant past rejected drafts; their slots are overwritten.  Nothing depends on
        the host, so _run_steps captures and replays the step; the host polls the status words every 8th step (behind `done` a step rewrites the same assistant
        slots, stages no candidate and accepts nothing).  assist_on_device = False, or an assistant outside the single-sequence chain: the same rules in torch
        ops with host reads around the same verify forward, eagerly.  self.last_assist_stats: {emitted, steps, accepted, rejecting} of the call, `launched`
        (the steps enqueued: up to seven more than `steps` on the device route) and `drafted` (k per step that was open)."""
        dev, S0, k, am = self.device_, ids.shape[1], assist.k, assist.model
        M = k + 1
        am._require_hip()
        lo_a, padded, Ka, Va, pos_rows, krange, fast = am._prefill_setup(attention_mask, 1, S0, max_new + k + 1, "generate(assistant_model=...)")
        am._decode_layers(am._merged_embeddings(ids, input_features, input_features_mask), 1, S0, 0, (Ka, Va), pos_rows, krange, fast, kv_lo=lo_a if padded else None)
        head, emb = self.arena["lm_head.weight"].data, self.arena[self._lm + "embed_tokens.weight"].data
        state = torch.cat([lo, torch.tensor([S0 + 1, S0], device=dev, dtype=torch.int32), S0 - lo]).contiguous()   # [lo, key-range end, cache slot, position]
        ls = _lookup.build_state(_lookup.LookupSpec(k, 1), ids, self._select_token(first_logits), max_new, eos, state, emb.shape[1])
        aws = self._decode_attn_workspace(dev, cache[1].shape[4], M) if self._lookup_chain_ok(M, head) else None
        a = _assist.build_state(am, k, (Ka, Va), dev)
        on_device = self.assist_on_device and a.aws is not None
        verify = lambda: self._lookup_forward(ls["x"], cache, ls["pos"], ls["krange"], state[2:3], aws, head)

        def step():
            _assist.begin(ls, a)
            for j in range(M):
                x = am._chain_layers(a.x0, a.cache, a.dstate[3:4], a.dstate[0:2], a.dstate[2:3], aws=a.aws)
                if j == k:   # the last draft's keys only: no lm_head, no selection
                    break
                am._chain_lm_head(x, a.head, part_val=a.part_val, part_idx=a.part_idx)
                _lib.call("afk_decode_select_greedy", a.part_val.data_ptr(), a.part_idx.data_ptr(), a.part_val.numel(), a.nxt.data_ptr(), a.draft.data_ptr(), 0,
                          a.dstate.data_ptr(), a.emb.data_ptr(), a.emb.stride(0), a.emb.shape[1], a.x0.data_ptr(), ops._stream())
            _assist.stage(ls, a, emb)
            _lookup.accept(ls, verify())

        def host_step():
            _assist.begin_host(ls, a)
            cur = int(a.dstate[2])
            for j in range(M):
                logits = am._decode_logits(dst)   # appends the keys of a.nxt at slot dstate[2]
                a.dstate[1:4] += 1
                if j == k:
                    break
                a.nxt.copy_(self._select_token(logits))
                a.draft[cur + j] = a.nxt[0]
            _assist.stage_host(ls, a, emb)
            _lookup.accept_host(ls, verify())

        done = lambda t=0: ls["status"].tolist()[_lookup.DONE] != 0   # one small copy
        launched = 0
        if on_device:
            launched = _run_steps(step, max_new, use_graph, done)
        else:
            dst = am._new_state(a.cache, lo_a, S0, a.nxt, aws=a.aws)
            dst.cur, dst.single = a.dstate[2:3], SingleSequence(state=a.dstate, kr1=a.dstate[0:2], pos1=a.dstate[3:4], advance=a.dstate[1:4])
            while not done():
                host_step()
                launched += 1
        st = ls["status"].tolist()
        self.last_assist_stats = dict(emitted=st[_lookup.EMITTED], steps=st[_lookup.STEPS], accepted=st[_lookup.ACCEPTED], rejecting=st[_lookup.REJECTING],
                                      launched=launched, drafted=k * st[_lookup.STEPS])
        return torch.cat([ids, ls["tokens"][None, :st[_lookup.EMITTED]]], dim=1)

    @staticmethod
    def _generate_output(flags, sequences, S0, rec, cache, lo, shared=None, cfg=None):
        """what generate() returns: the plain sequences, or under return_dict_in_generate the AfkGenerateOutput around them - n = generated columns, scores /
        logits = the first n slots of the recorded buffers as tuples of [B, V] views, past_key_values = the cache of every token but the last (shared: `cache` is
        the tail cache and lo is per continuation - the two caches are laid out as one plain cache of B * n rows, decode_share.materialize; cfg:
        `cache` has 2 * B rows and the B conditional ones are copied out, decode_cfg.materialize)"""
        if not flags.return_dict:
            return sequences
        from .generation_output import AfkGenerateOutput
        from .modeling import AfkKVCache

        n = sequences.shape[1] - S0
        rows = lambda k: tuple(rec[k][i] for i in range(n)) if rec and rec.get(k) is not None else None
        logits = rows("logits")
        scores = logits if (rec and rec.get("scores") is not None and rec["scores"] is rec.get("logits")) else rows("scores")   # the same tensor objects, as the reference
        if cfg is not None:   # the conditional rows alone, at the slots a plain call would hold them in (the reference returns the conditional cache)
            kv = _cfg.materialize(cache[0], cache[1], lo, cfg, S0 + n - 1)
        elif shared is not None:
            kv = _share.materialize(shared.cache[0], shared.cache[1], lo[::shared.n], S0, cache[0], cache[1], shared.n, S0 + n - 1)
        else:
            kv = AfkKVCache(cache[0], cache[1], lo, S0 + n - 1)
        return AfkGenerateOutput(sequences=sequences, scores=scores, logits=logits, past_key_values=kv)

    def compute_transition_scores(self, sequences, scores, beam_indices=None, normalize_logits=False):
        """GenerationMixin.compute_transition_scores (transformers/generation/utils.py:1433-1555) for greedy / sampled outputs: [B, len(scores)] fp32, the
        score of every generated token (the last len(scores) columns of `sequences`) in `scores` - or `logits` - as generate(return_dict_in_generate=True)
        returned them; normalize_logits: minus the row's logsumexp, i.e. log-probabilities (-inf entries, the tokens a processor or warper removed, count as
        probability 0).  One launch (afk_transition_scores); tuples that are consecutive views of one buffer - what generate() returns - are read in place,
        anything else is stacked first.  beam_indices: beam-search outputs are not produced by this implementation's generate() and are refused."""
        if beam_indices is not None:
            raise AfkError("compute_transition_scores(beam_indices=...) is not supported: generate() returns no beam-search outputs")
        from .generation_output import step_buffer_view

        scores = tuple(scores)
        if not scores:
            raise AfkError("compute_transition_scores: `scores` is empty")
        if sequences.dim() != 2 or sequences.shape[1] < len(scores) or sequences.shape[0] != scores[0].shape[0]:
            raise AfkError(f"compute_transition_scores: sequences {tuple(sequences.shape)} do not hold {len(scores)} generated columns for {scores[0].shape[0]} rows")
        buf = step_buffer_view(scores) if scores[0].is_cuda else None
        if buf is None:
            buf = torch.stack([s.to(self.device_, torch.float32) for s in scores]).contiguous()
        tokens = sequences[:, sequences.shape[1] - len(scores):].to(buf.device, torch.int64).contiguous()
        return ops.transition_scores(buf, tokens, normalize=bool(normalize_logits))

    @torch.no_grad()
    def _generate_with_hooks(self, ids, st, logits, max_new, procs, criteria, streamer, eos, pad):
        """GenerationMixin._sample's loop with its per-step callbacks (transformers/generation/utils.py:2730-2830): scores = logits_processor(input_ids,
        logits); token = argmax / multinomial; finished rows emit pad; streamer.put(tokens) (the prompt first, streamer.end() at the end);
        a row finishes on EOS or when stopping_criteria(input_ids, scores) says so.  Host code runs between the steps, so they are enqueued eagerly
        (no HIP graph) - the decode kernels are the ones of the graph path, and a sampled token is draw t of afk_decode_sample on the PROCESSED scores (a
        token a processor set to -inf is never drawn), the same draw the graph path makes for token t.  eos: the ids as a tuple, pad: decode_stop.resolve's."""
        B = ids.shape[0]
        dev = ids.device
        eos = torch.tensor(eos, device=dev) if eos else None
        pad = pad if pad is not None else 0
        done = torch.zeros(B, device=dev, dtype=torch.bool)
        stop = st.stop
        seq = ids
        if streamer is not None:
            streamer.put(ids.cpu())
        for t in range(max_new):
            if t > 0:
                logits, uncond, _ = self._guided_rows(st, self._decode_logits(st))        # appends the K / V of st.nxt at the cache slot st.cur
                (st.single.advance if st.single is not None else st.cur).add_(1)
                self._record_and_process(st, logits, step_off=t, uncond=uncond)   # guidance, then the built-in processors: st.nxt is token t - 1 as appended to seq (pad for a finished row)
                if procs:
                    logits = procs(seq, logits)
            # token 0 is drawn a second time here (generate() drew it for st.nxt): the same draw, the same scores row - which generate() has recorded where it is greedy
            tok = self._pick_token(st, logits, step_off=t, record=t > 0)
            tok = torch.where(done, torch.full_like(tok, pad), tok)
            if stop is not None:   # the device rule (eos list, stop strings), eagerly and in front of the user's criteria; token 0 was judged by generate() - the same answer
                tok = tok.contiguous()
                _stop.apply(stop, tok, step_off=t, feed_pad=True)
            seq = torch.cat([seq, tok[:, None]], dim=1)
            if streamer is not None:
                streamer.put(tok.cpu())
            if stop is not None:
                done = done | (stop["stop_at"] <= t)
            elif eos is not None:
                done = done | torch.isin(tok, eos)
            if criteria:
                r = criteria(seq, logits)
                done = done | (r.to(dev).reshape(-1).bool() if torch.is_tensor(r) else torch.full_like(done, bool(r)))
            if bool(done.all()):
                break
            st.nxt.copy_(tok if st.cfg is None else torch.cat([tok, tok]))   # guidance: both rows of a pair are fed the token (pad for a finished row)
        if streamer is not None:
            streamer.end()
        return seq

    @torch.no_grad()
    def _generate_recompute(self, ids, input_features, input_features_mask, attention_mask, max_new_tokens, eos):
        """reference path without a cache (every step re-runs the whole prefix through forward()): used by the tests to pin the cache path.  eos: a tuple"""
        if ids.shape[0] != 1 and attention_mask is not None and not bool(attention_mask.all()):
            raise AfkError("the recompute path does not support padded batches")
        eos = torch.tensor(eos, device=ids.device) if eos else None
        for _ in range(max_new_tokens):
            out = self.forward(input_ids=ids, input_features=input_features, input_features_mask=input_features_mask, logits_to_keep=1)
            nxt = out.logits[:, -1, :].float().argmax(-1, keepdim=True)
            ids = torch.cat([ids, nxt], dim=1)
            if eos is not None and bool(torch.isin(nxt, eos).all()):
                break
        return ids
