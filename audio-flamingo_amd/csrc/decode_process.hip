// Logits processors of the decode step on the device (generate(repetition_penalty / no_repeat_ngram_size / min_new_tokens / suppress_tokens /
// begin_suppress_tokens)): the processors GenerationMixin._get_logits_processor (transformers/generation/utils.py:1174-1290) puts in front of the warpers, one
// launch, no host state - the step can be captured into a HIP graph with them.  Oracle: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
// MinNewTokensLengthLogitsProcessor, SuppressTokensLogitsProcessor and SuppressTokensAtBeginLogitsProcessor (transformers/generation/logits_process.py).
//
// One 1024-thread block per row.  What the reference reads from `input_ids` lives on the device: hist[b] holds the prompt ids and, behind them, every token
// selected so far; seen[b] is a bitmap over the vocabulary with one bit per id that occurs in hist[b].  The launch for token t first appends token t - 1 (the
// next_token buffer the selection launch of the previous step wrote) - thread 0 stores it and sets its bit, and every thread also carries it in a register, so
// nothing the block reads depends on that store having landed.  The penalty walks the bitmap: one read-modify-write per DISTINCT id, whoever owns the word, so an
// id that occurs twice is penalised once.  The n-gram bans and the id-list bans only store -inf: they commute with each other and follow the penalty behind a
// block barrier.  With `select` the same block then takes the argmax of the row it just wrote (one sequence) and does the greedy launch's bookkeeping.
//
// afk_decode_process_ex is the same kernel compiled with the other built-in processors in their places (generate(sequence_bias / bad_words_ids / min_length /
// forced_eos_token_id / exponential_decay_length_penalty); oracle: SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor, MinLengthLogitsProcessor,
// ForcedEOSTokenLogitsProcessor, ExponentialDecayLengthPenalty).  These do arithmetic on the row an earlier stage left, so each of them sits between block
// barriers.  A sequence table is grouped by last id on the host: one thread walks one group and adds its biases in the table's order, so the fp32 sum has one
// order and needs no atomics.  Forced EOS and the length penalty both map an entry to a function of that entry alone, so one pass over the row applies the
// two in their order per entry; the barriers stand in front of and behind that pass.
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr int NT = 1024, NW = NT / 64, LU = 8;

struct ProcessArgs {
    float* logits; int64_t ld; int V; int* hist; int64_t ld_hist; int S0; unsigned int* seen; int64_t ld_seen; const int* step_base; int step_off;
    long long* next_token; float penalty; int g; const int* sup; int nsup; const int* bsup; int nbsup; const int* eos; int neos; int min_new; int select;
    long long* tokens_out; int tok_off; int* state; const bf16* emb; int64_t ld_emb; int H; bf16* x_out;
};

// sequences of a bias table, grouped by last id: group g biases id group_id[g] by l1[g] (its one-id sequence, 0.0f without one) and by the sequences
// group_off[g] .. group_off[g + 1), sequence s = the ids[seq_off[s] .. seq_off[s + 1]) in front of that last id with the bias seq_bias[s]
struct SeqTable {
    const int* ids; const int* seq_off; const float* seq_bias; const int* group_id; const float* group_l1; const int* group_off; int n_groups;
};

struct ExArgs {
    SeqTable bias, bad; int min_length; const int* forced; int nforced; const float* decay; int ndecay; int decay_start; int max_new;
};

__device__ __forceinline__ bool holds(const int* list, int n, int id) {
    bool in = false;
    for (int k = 0; k < n; ++k) in |= list[k] == id;
    return in;
}

// x + |x| * c as the reference computes it: the product rounded, then the sum rounded - never contracted into one fused multiply-add
__device__ __forceinline__ float add_scaled_abs(float x, float c) {
#pragma clang fp contract(off)
    const float m = fabsf(x) * c;
    return x + m;
}

// SequenceBiasLogitsProcessor.__call__ on one row with a history of n ids: x = x + acc on every entry.  acc is 0.0f outside the groups and never -0.0f (it
// starts from +0.0f), so adding 0.0f everywhere first and a group's acc behind a barrier gives the bits of the one add.  Ends behind a barrier.
template <class IdAt>
__device__ __forceinline__ void sequence_bias(float* row, int V, const SeqTable& tb, int n, IdAt id_at, int t) {
    for (int i = t; i < V; i += NT) row[i] = row[i] + 0.0f;
    __syncthreads();
    for (int g = t; g < tb.n_groups; g += NT) {
        const int id = tb.group_id[g];
        if (id < 0 || id >= V) continue;
        float acc = 0.0f + tb.group_l1[g];
        for (int s = tb.group_off[g]; s < tb.group_off[g + 1]; ++s) {
            const int o = tb.seq_off[s], P = tb.seq_off[s + 1] - o;   // P = L - 1 ids in front of the last one
            bool same = P < n;                                        // L <= cur_len
            for (int k = 0; k < P && same; ++k) same = id_at(n - P + k) == tb.ids[o + k];
            acc += same ? tb.seq_bias[s] : 0.0f;
        }
        row[id] = row[id] + acc;
    }
    __syncthreads();
}

__device__ __forceinline__ void better(float& bv, int& bi, float v, int i) {   // larger value, then lower id; a NaN never wins (as decode_select_greedy_kernel)
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

template <bool EX>
__global__ __launch_bounds__(NT) void decode_process_kernel(ProcessArgs a, ExArgs e) {
    __shared__ float sv[NW];
    __shared__ int si[NW];
    __shared__ int s_step, s_tok;
    const int t = threadIdx.x, b = blockIdx.x, V = a.V;
    if (t == 0) s_step = (a.step_base ? *a.step_base : 0) + a.step_off;   // read before the bookkeeping below advances the state it may live in
    __syncthreads();
    const int step = max(s_step, 0);
    float* row = a.logits + (int64_t)b * a.ld;
    int* hist = a.hist + (int64_t)b * a.ld_hist;
    unsigned int* seen = a.seen + (int64_t)b * a.ld_seen;
    const int64_t n64 = (int64_t)a.S0 + step;
    const int n = (int)(n64 < a.ld_hist ? n64 : a.ld_hist);   // never past the history buffer (the entry point checks what the host can know)

    // ---- step 0: the token selected last joins the history and the seen set
    int prev = -1, prev_at = -1;
    if (step >= 1 && n64 <= a.ld_hist) {
        prev = (int)a.next_token[b];
        prev_at = n - 1;
        if (t == 0) {
            hist[prev_at] = prev;
            if (prev >= 0 && prev < V) atomicOr(&seen[prev >> 5], 1u << (prev & 31));
        }
    }
    const bool prev_ok = prev >= 0 && prev < V;
    auto id_at = [&](int j) { return j == prev_at ? prev : hist[j]; };

    // ---- sequence bias, in front of the penalty (which scales what it added)
    if constexpr (EX)
        if (e.bias.n_groups > 0) sequence_bias(row, V, e.bias, n, id_at, t);

    // ---- step 1: repetition penalty, once per distinct id
    const float p = a.penalty;
    if (p != 1.f) {
        const int nwords = (V + 31) >> 5;
        for (int w = t; w < nwords; w += NT) {
            unsigned int bits = seen[w];
            if (prev_ok && (prev >> 5) == w) bits |= 1u << (prev & 31);
            while (bits) {
                const int i = (w << 5) + __ffs((int)bits) - 1;
                bits &= bits - 1;
                if (i < V) {
                    const float x = row[i];
                    row[i] = x < 0.f ? x * p : x / p;
                }
            }
        }
    }
    __syncthreads();

    // ---- step 2: no-repeat n-gram: whatever followed an earlier occurrence of the last g - 1 ids
    const int g = a.g;
    if (g > 0 && n + 1 >= g) {
        const int tail = n - g + 1;
        for (int j = t; j <= n - g; j += NT) {
            bool same = true;
            for (int k = 0; k < g - 1 && same; ++k) same = id_at(j + k) == id_at(tail + k);
            if (same) {
                const int id = id_at(j + g - 1);
                if (id >= 0 && id < V) row[id] = -INFINITY;
            }
        }
    }
    if constexpr (EX) {
        // ---- bad words: a sequence table whose biases are -inf, on the row the n-gram bans left
        if (e.bad.n_groups > 0) {
            __syncthreads();
            sequence_bias(row, V, e.bad, n, id_at, t);
        }
        // ---- min_length and min_new_tokens: the eos ids
        if (n64 < e.min_length || step < a.min_new)
            for (int i = t; i < a.neos; i += NT) {
                const int id = a.eos[i];
                if (id >= 0 && id < V) row[id] = -INFINITY;
            }
        // ---- forced EOS at the last token, then the exponential length penalty: each entry from its own value, in one pass
        const bool forced = e.nforced > 0 && s_step == e.max_new - 1;
        const bool decay = e.decay && a.neos > 0 && step > e.decay_start;
        if (forced || decay) {
            const float c = decay ? e.decay[min(step, e.ndecay - 1)] : 0.f;
            __syncthreads();
            for (int i = t; i < V; i += NT) {
                float x = row[i];
                if (forced) x = holds(e.forced, e.nforced, i) ? 0.f : -INFINITY;
                if (decay) x = holds(a.eos, a.neos, i) ? add_scaled_abs(x, c) : x + 0.0f;
                row[i] = x;
            }
            __syncthreads();
        }
    }
    // ---- step 3: bans
    for (int i = t; i < a.nsup; i += NT) {
        const int id = a.sup[i];
        if (id >= 0 && id < V) row[id] = -INFINITY;
    }
    if (step == 0)
        for (int i = t; i < a.nbsup; i += NT) {
            const int id = a.bsup[i];
            if (id >= 0 && id < V) row[id] = -INFINITY;
        }
    if constexpr (!EX)
        if (step < a.min_new)
            for (int i = t; i < a.neos; i += NT) {
                const int id = a.eos[i];
                if (id >= 0 && id < V) row[id] = -INFINITY;
            }
    if (!a.select) return;

    // ---- greedy selection on the processed row + the bookkeeping block of decode_select_greedy_kernel (one sequence)
    __syncthreads();
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int base = 0; base < V; base += LU * NT) {
        float x[LU];
#pragma unroll
        for (int u = 0; u < LU; ++u) x[u] = row[min(base + u * NT + t, V - 1)];   // clamped: a repeated element never changes the result
#pragma unroll
        for (int u = 0; u < LU; ++u) better(bv, bi, x[u], min(base + u * NT + t, V - 1));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        better(bv, bi, ov, oi);
    }
    if ((t & 63) == 0) { sv[t >> 6] = bv; si[t >> 6] = bi; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < NW; ++w) better(bv, bi, sv[w], si[w]);
        if (bi == 0x7fffffff) bi = 0;   // no logit that compares (all NaN): 0; an all -inf row answers 0 as the lowest id of the tie
        s_tok = bi;
        a.next_token[0] = bi;
        if (a.tokens_out) a.tokens_out[a.state[2] + a.tok_off] = bi;
        a.state[1] += 1;   // key-range end
        a.state[2] += 1;   // cache slot of the next token
        a.state[3] += 1;   // its position
    }
    __syncthreads();
    const bf16* erow = a.emb + (int64_t)s_tok * a.ld_emb;
    for (int k = t * 4; k < a.H; k += 4 * NT) *(bf16x4*)(a.x_out + k) = *(const bf16x4*)(erow + k);
}

}  // namespace

#define ST ((hipStream_t)stream)

// the checks and the argument record both entry points share; `who` names the entry in the message
static int process_args(const char* who, ProcessArgs& a, float* logits, int64_t ld_logits, int B, int V, int* hist, int64_t ld_hist, int S0, unsigned int* seen,
                        int64_t ld_seen, const int* step_base, int step_off, int64_t* next_token, float penalty, int no_repeat_ngram_size, const int* suppress,
                        int n_suppress, const int* begin_suppress, int n_begin_suppress, const int* eos, int n_eos, int min_new_tokens, int select,
                        int64_t* tokens_out, int tok_off, int* state, const void* emb, int64_t ld_emb, int H, void* x_out) {
    AFK_REQUIRE(logits && hist && seen, "%s: null pointer (logits, hist, seen)", who);
    AFK_REQUIRE(next_token || (!step_base && step_off == 0 && !select), "%s: null pointer (next_token: only token 0 of a run without selection has none)", who);
    AFK_REQUIRE(B >= 1 && V >= 1 && ld_logits >= V && ld_seen >= (V + 31) / 32 && S0 >= 0 && ld_hist >= 1,
                "%s: unsupported shape (B >= 1, V >= 1, ld_logits >= V, ld_seen >= ceil(V / 32), S0 >= 0)", who);
    AFK_REQUIRE(penalty > 0.f && penalty <= 3.0e38f, "%s: penalty %g (finite, penalty > 0)", who, (double)penalty);
    AFK_REQUIRE(no_repeat_ngram_size >= 0, "%s: no_repeat_ngram_size %d (>= 0; 0 switches it off)", who, no_repeat_ngram_size);
    AFK_REQUIRE(n_suppress >= 0 && n_begin_suppress >= 0 && n_eos >= 0 && (suppress || !n_suppress) && (begin_suppress || !n_begin_suppress) && (eos || !n_eos),
                "%s: an id list with a count and a null pointer", who);
    AFK_REQUIRE(S0 <= ld_hist && (step_base || (step_off >= 0 && (int64_t)S0 + step_off <= ld_hist)),
                "%s: history of S0 + t = %d + %d ids in a buffer of %lld (S0 + t <= ld_hist)", who, S0, step_off, (long long)ld_hist);
    AFK_REQUIRE(!select || (B == 1 && state && emb && x_out && H > 0 && H % 4 == 0 && ld_emb % 4 == 0),
                "%s: the selection block (select) needs B == 1, state, emb, x_out and H %% 4 == 0", who);
    a = {logits, ld_logits, V, hist, ld_hist, S0, seen, ld_seen, step_base, step_off, (long long*)next_token, penalty, no_repeat_ngram_size, suppress,
         n_suppress, begin_suppress, n_begin_suppress, eos, n_eos, min_new_tokens, select, (long long*)tokens_out, tok_off, state, (const bf16*)emb,
         ld_emb, H, (bf16*)x_out};
    return AFK_OK;
}

extern "C" int afk_decode_process(float* logits, int64_t ld_logits, int B, int V, int* hist, int64_t ld_hist, int S0, unsigned int* seen, int64_t ld_seen,
                                  const int* step_base, int step_off, int64_t* next_token, float penalty, int no_repeat_ngram_size, const int* suppress,
                                  int n_suppress, const int* begin_suppress, int n_begin_suppress, const int* eos, int n_eos, int min_new_tokens, int select,
                                  int64_t* tokens_out, int tok_off, int* state, const void* emb, int64_t ld_emb, int H, void* x_out, void* stream) {
    ProcessArgs a;
    const int rc = process_args("afk_decode_process", a, logits, ld_logits, B, V, hist, ld_hist, S0, seen, ld_seen, step_base, step_off, next_token, penalty,
                                no_repeat_ngram_size, suppress, n_suppress, begin_suppress, n_begin_suppress, eos, n_eos, min_new_tokens, select, tokens_out,
                                tok_off, state, emb, ld_emb, H, x_out);
    if (rc != AFK_OK) return rc;
    hipLaunchKernelGGL(decode_process_kernel<false>, dim3(B), dim3(NT), 0, ST, a, ExArgs{});
    AFK_LAUNCH_CHECK("afk_decode_process");
    return AFK_OK;
}

extern "C" int afk_decode_process_ex(float* logits, int64_t ld_logits, int B, int V, int* hist, int64_t ld_hist, int S0, unsigned int* seen, int64_t ld_seen,
                                     const int* step_base, int step_off, int64_t* next_token, float penalty, int no_repeat_ngram_size, const int* suppress,
                                     int n_suppress, const int* begin_suppress, int n_begin_suppress, const int* eos, int n_eos, int min_new_tokens, int select,
                                     int64_t* tokens_out, int tok_off, int* state, const void* emb, int64_t ld_emb, int H, void* x_out, const int* bias_ids,
                                     const int* bias_seq_off, const float* bias_seq_bias, int n_bias_seqs, const int* bias_group_id, const float* bias_group_l1,
                                     const int* bias_group_off, int n_bias_groups, const int* bad_ids, const int* bad_seq_off, const float* bad_seq_bias,
                                     int n_bad_seqs, const int* bad_group_id, const float* bad_group_l1, const int* bad_group_off, int n_bad_groups,
                                     int min_length, const int* forced_eos, int n_forced_eos, const float* decay, int n_decay, int decay_start,
                                     int max_new_tokens, void* stream) {
    ProcessArgs a;
    const int rc = process_args("afk_decode_process_ex", a, logits, ld_logits, B, V, hist, ld_hist, S0, seen, ld_seen, step_base, step_off, next_token, penalty,
                                no_repeat_ngram_size, suppress, n_suppress, begin_suppress, n_begin_suppress, eos, n_eos, min_new_tokens, select, tokens_out,
                                tok_off, state, emb, ld_emb, H, x_out);
    if (rc != AFK_OK) return rc;
    AFK_REQUIRE(n_bias_seqs >= 0 && n_bias_groups >= 0 && (!n_bias_seqs || (n_bias_groups && bias_ids && bias_seq_off && bias_seq_bias)) &&
                    (!n_bias_groups || (bias_group_id && bias_group_l1 && bias_group_off)),
                "afk_decode_process_ex: the sequence_bias table has counts (%d sequences in %d groups) and a null pointer", n_bias_seqs, n_bias_groups);
    AFK_REQUIRE(n_bad_seqs >= 0 && n_bad_groups >= 0 && (!n_bad_seqs || (n_bad_groups && bad_ids && bad_seq_off && bad_seq_bias)) &&
                    (!n_bad_groups || (bad_group_id && bad_group_l1 && bad_group_off)),
                "afk_decode_process_ex: the bad_words table has counts (%d sequences in %d groups) and a null pointer", n_bad_seqs, n_bad_groups);
    AFK_REQUIRE(n_forced_eos >= 0 && (forced_eos || !n_forced_eos), "afk_decode_process_ex: forced_eos with a count and a null pointer");
    AFK_REQUIRE(max_new_tokens >= 1 && min_length >= 0, "afk_decode_process_ex: max_new_tokens %d (>= 1), min_length %d (>= 0)", max_new_tokens, min_length);
    AFK_REQUIRE(!decay || n_decay >= max_new_tokens, "afk_decode_process_ex: a decay table of %d entries for max_new_tokens %d (one per token)", n_decay,
                max_new_tokens);
    AFK_REQUIRE(decay || !n_decay, "afk_decode_process_ex: decay with a count and a null pointer");
    ExArgs e = {{bias_ids, bias_seq_off, bias_seq_bias, bias_group_id, bias_group_l1, bias_group_off, n_bias_groups},
                {bad_ids, bad_seq_off, bad_seq_bias, bad_group_id, bad_group_l1, bad_group_off, n_bad_groups},
                min_length, forced_eos, n_forced_eos, decay, n_decay, decay_start, max_new_tokens};
    hipLaunchKernelGGL(decode_process_kernel<true>, dim3(B), dim3(NT), 0, ST, a, e);
    AFK_LAUNCH_CHECK("afk_decode_process_ex");
    return AFK_OK;
}
