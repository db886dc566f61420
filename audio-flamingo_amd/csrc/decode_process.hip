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
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr int NT = 1024, NW = NT / 64, LU = 8;

struct ProcessArgs {
    float* logits; int64_t ld; int V; int* hist; int64_t ld_hist; int S0; unsigned int* seen; int64_t ld_seen; const int* step_base; int step_off;
    long long* next_token; float penalty; int g; const int* sup; int nsup; const int* bsup; int nbsup; const int* eos; int neos; int min_new; int select;
    long long* tokens_out; int tok_off; int* state; const bf16* emb; int64_t ld_emb; int H; bf16* x_out;
};

__device__ __forceinline__ void better(float& bv, int& bi, float v, int i) {   // larger value, then lower id; a NaN never wins (as decode_select_greedy_kernel)
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

__global__ __launch_bounds__(NT) void decode_process_kernel(ProcessArgs a) {
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

extern "C" int afk_decode_process(float* logits, int64_t ld_logits, int B, int V, int* hist, int64_t ld_hist, int S0, unsigned int* seen, int64_t ld_seen,
                                  const int* step_base, int step_off, int64_t* next_token, float penalty, int no_repeat_ngram_size, const int* suppress,
                                  int n_suppress, const int* begin_suppress, int n_begin_suppress, const int* eos, int n_eos, int min_new_tokens, int select,
                                  int64_t* tokens_out, int tok_off, int* state, const void* emb, int64_t ld_emb, int H, void* x_out, void* stream) {
    AFK_REQUIRE(logits && hist && seen, "afk_decode_process: null pointer (logits, hist, seen)");
    AFK_REQUIRE(next_token || (!step_base && step_off == 0 && !select), "afk_decode_process: null pointer (next_token: only token 0 of a run without selection has none)");
    AFK_REQUIRE(B >= 1 && V >= 1 && ld_logits >= V && ld_seen >= (V + 31) / 32 && S0 >= 0 && ld_hist >= 1,
                "afk_decode_process: unsupported shape (B >= 1, V >= 1, ld_logits >= V, ld_seen >= ceil(V / 32), S0 >= 0)");
    AFK_REQUIRE(penalty > 0.f && penalty <= 3.0e38f, "afk_decode_process: penalty %g (finite, penalty > 0)", (double)penalty);
    AFK_REQUIRE(no_repeat_ngram_size >= 0, "afk_decode_process: no_repeat_ngram_size %d (>= 0; 0 switches it off)", no_repeat_ngram_size);
    AFK_REQUIRE(n_suppress >= 0 && n_begin_suppress >= 0 && n_eos >= 0 && (suppress || !n_suppress) && (begin_suppress || !n_begin_suppress) && (eos || !n_eos),
                "afk_decode_process: an id list with a count and a null pointer");
    AFK_REQUIRE(S0 <= ld_hist && (step_base || (step_off >= 0 && (int64_t)S0 + step_off <= ld_hist)),
                "afk_decode_process: history of S0 + t = %d + %d ids in a buffer of %lld (S0 + t <= ld_hist)", S0, step_off, (long long)ld_hist);
    AFK_REQUIRE(!select || (B == 1 && state && emb && x_out && H > 0 && H % 4 == 0 && ld_emb % 4 == 0),
                "afk_decode_process: the selection block (select) needs B == 1, state, emb, x_out and H %% 4 == 0");
    ProcessArgs a = {logits, ld_logits, V, hist, ld_hist, S0, seen, ld_seen, step_base, step_off, (long long*)next_token, penalty, no_repeat_ngram_size, suppress,
                     n_suppress, begin_suppress, n_begin_suppress, eos, n_eos, min_new_tokens, select, (long long*)tokens_out, tok_off, state, (const bf16*)emb,
                     ld_emb, H, (bf16*)x_out};
    hipLaunchKernelGGL(decode_process_kernel, dim3(B), dim3(NT), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_decode_process");
    return AFK_OK;
}
