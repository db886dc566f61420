// Prompt-lookup decoding on the device (generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n)): the two decisions GenerationMixin._assisted_decoding
// takes on the host around its verify forward - which tokens to draft (PromptLookupCandidateGenerator.get_candidates, transformers/generation/
// candidate_generator.py:1057-1150) and how many of them the model's own argmaxes confirm (the greedy branch of transformers/generation/utils.py:3771-3786) -
// as launches with no host state, so that draft -> verify forward -> accept is one capturable step.  The contract is in include/afk.h.
//
// Both are index work on a few thousand integers (the draft) or M rows of logits (the accept): one block each, apart from the row argmaxes, which
// AFK_LOOKUP_PARTS blocks per row take in slices.  Nothing in a launch waits for another block: the argmax slices and their fold are two kernels of one call.
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr int DRAFT_NT = 1024, ARG_NT = 256, INT_MAX_ = 0x7fffffff;
enum { W_LEN = 0, W_EMITTED = 1, W_DONE = 2, W_NCAND = 3, W_STEPS = 4, W_ACCEPTED = 5, W_REJECTING = 6, W_NMATCH = 7 };

__device__ inline bool is_eos(int tok, const int* eos, int n_eos) {
    for (int i = 0; i < n_eos; ++i)
        if (eos[i] == tok) return true;
    return false;
}

struct DraftArgs {
    const int* ids; int ids_cap; int* status; const int* state; int k; int ngram; int max_new; const int* eos; int n_eos;
    int* cand; long long* rows; int* pos; int* krange; const bf16* emb; int64_t ld_emb; int vocab; int H; bf16* x_out; int64_t ldx;
};

// A window that ends in front of position e (its continuation starts at e) matches the trailing g-gram exactly when the g ids in front of e equal the g ids in
// front of len.  So one walk over e = 1 .. len - 1 serves every g at once: L(e) = the number of ids in front of e that agree with the tail, and e is a match for
// g = 1 .. L(e).  The leftmost window of size g is the smallest such e; e < len is the "non-empty continuation" condition, which also rules the tail itself out.
__global__ __launch_bounds__(DRAFT_NT) void lookup_draft_kernel(DraftArgs a) {
    __shared__ int s_best[AFK_LOOKUP_MAX_NGRAM + 1];
    __shared__ int s_tail[AFK_LOOKUP_MAX_NGRAM];
    __shared__ int s_tok[AFK_LOOKUP_MAX_K + 1];
    const int t = threadIdx.x;
    const int len = min(max(a.status[W_LEN], 1), a.ids_cap);
    const int budget = a.max_new - a.status[W_EMITTED] - 1;   // a step emits its accepted candidates and one more token
    const bool open = a.status[W_DONE] == 0 && budget > 0;
    const int nmax = min(a.ngram, len - 1);
    if (t < nmax) s_tail[t] = a.ids[len - 1 - t];
    if (t <= AFK_LOOKUP_MAX_NGRAM) s_best[t] = INT_MAX_;
    __syncthreads();
    if (open) {
        for (int e = 1 + t; e < len; e += DRAFT_NT) {
            const int lim = min(nmax, e);
            int L = 0;
            while (L < lim && a.ids[e - 1 - L] == s_tail[L]) ++L;
            for (int g = 1; g <= L; ++g) atomicMin(&s_best[g], e);
        }
    }
    __syncthreads();
    if (t == 0) {
        const int last = a.ids[len - 1];
        int n_cand = 0, start = 0;
        if (open) {
            for (int g = nmax; g >= 1; --g) {
                if (s_best[g] == INT_MAX_) continue;
                start = s_best[g];
                int n = min(min(a.k, len - start), budget);
                for (int i = 0; i < n; ++i)
                    if (is_eos(a.ids[start + i], a.eos, a.n_eos)) { n = i; break; }   // cropped in front of the first eos id (:1132-1137)
                n_cand = n;   // nothing left: no candidates - the reference tries no other match either (:1138-1144)
                break;
            }
        }
        s_tok[0] = last;
        for (int i = 0; i < a.k; ++i) {
            const int c = i < n_cand ? a.ids[start + i] : last;   // rows behind n_cand run on a valid id; nobody reads their logits
            a.cand[i] = c;
            s_tok[i + 1] = c;
        }
        a.status[W_NCAND] = n_cand;
    }
    __syncthreads();
    const int M = a.k + 1;
    if (t < M) {
        a.rows[t] = s_tok[t];
        a.pos[t] = a.state[3] + t;
        a.krange[2 * t] = a.state[0];
        a.krange[2 * t + 1] = a.state[1] + t;   // row j sees the cache up to its own slot: a staircase over one sequence
    }
    if (a.x_out == nullptr) return;
    const int pieces = a.H / 8;
    for (int i = t; i < M * pieces; i += DRAFT_NT) {
        const int j = i / pieces, c = i % pieces;
        const int tok = min(max(s_tok[j], 0), a.vocab - 1);
        *(bf16x8*)(a.x_out + (int64_t)j * a.ldx + c * 8) = *(const bf16x8*)(a.emb + (int64_t)tok * a.ld_emb + c * 8);
    }
}

// (max, argmax) of one slice of one row, afk_decode_select_greedy's order: the larger value, equal values -> the lower id; a NaN compares false and is never taken
__device__ inline void take(float v, int i, float& bv, int& bi) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

__global__ __launch_bounds__(ARG_NT) void lookup_argmax_kernel(const float* __restrict__ logits, int64_t ld, int V, int vec, const int* __restrict__ status,
                                                               float* __restrict__ part_val, int* __restrict__ part_idx) {
    __shared__ float sv[ARG_NT / 64];
    __shared__ int si[ARG_NT / 64];
    if (status[W_DONE] != 0) return;   // block-uniform: behind the end nothing is written, the scratch included
    const int part = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    const int per = ((V + AFK_LOOKUP_PARTS - 1) / AFK_LOOKUP_PARTS + 3) & ~3;
    const int c0 = min(part * per, V), c1 = min(c0 + per, V);
    const float* z = logits + (int64_t)row * ld;
    float bv = -INFINITY;
    int bi = INT_MAX_;
    if (vec) {   // V % 4 == 0 and 16-byte rows: c0 and c1 are multiples of four
        for (int i = c0 + 4 * t; i < c1; i += 4 * ARG_NT) {
            const f32x4 v = *(const f32x4*)(z + i);
#pragma unroll
            for (int u = 0; u < 4; ++u) take(v[u], i + u, bv, bi);
        }
    } else {
        for (int i = c0 + t; i < c1; i += ARG_NT) take(z[i], i, bv, bi);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        take(ov, oi, bv, bi);
    }
    if ((t & 63) == 0) { sv[t >> 6] = bv; si[t >> 6] = bi; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < ARG_NT / 64; ++w) take(sv[w], si[w], bv, bi);
        part_val[row * AFK_LOOKUP_PARTS + part] = bv;
        part_idx[row * AFK_LOOKUP_PARTS + part] = bi;
    }
}

struct AcceptArgs {
    int M; const int* cand; int* ids; int ids_cap; long long* tokens_out; int max_new; int* status; int* state; const int* eos; int n_eos; int* sel;
    const float* part_val; const int* part_idx;
};

__global__ __launch_bounds__(64) void lookup_accept_kernel(AcceptArgs a) {
    __shared__ int s_sel[AFK_LOOKUP_MAX_K + 1];
    if (a.status[W_DONE] != 0) return;   // block-uniform: replays behind the end change nothing
    const int t = threadIdx.x;
    if (t < a.M) {
        float bv = -INFINITY;
        int bi = INT_MAX_;
        for (int p = 0; p < AFK_LOOKUP_PARTS; ++p) take(a.part_val[t * AFK_LOOKUP_PARTS + p], a.part_idx[t * AFK_LOOKUP_PARTS + p], bv, bi);
        if (bi == INT_MAX_) bi = 0;   // nothing finite in the row: torch.argmax answers 0 for an all -inf row
        s_sel[t] = bi;
        a.sel[t] = bi;
    }
    __syncthreads();
    if (t != 0) return;
    const int len = a.status[W_LEN], emitted = a.status[W_EMITTED];
    const int n_cand = min(max(a.status[W_NCAND], 0), a.M - 1);
    int n_match = 0;
    while (n_match < n_cand && a.cand[n_match] == s_sel[n_match]) ++n_match;   // the leading candidates the model confirms (utils.py:3774)
    int e = min(min(n_match + 1, a.max_new - emitted), a.ids_cap - len);       // never past max_new_tokens (:3783-3786; the draft's crop already sees to it)
    bool hit = e <= 0;                                                         // a state with no room left (the caller's buffers are full) only closes
    e = max(e, 0);
    for (int i = 0; i < e; ++i)
        if (is_eos(s_sel[i], a.eos, a.n_eos)) { e = i + 1; hit = true; break; }
    for (int i = 0; i < e; ++i) {
        a.ids[len + i] = s_sel[i];
        if (a.tokens_out) a.tokens_out[emitted + i] = s_sel[i];
    }
    a.status[W_LEN] = len + e;
    a.status[W_EMITTED] = emitted + e;
    a.status[W_DONE] = (hit || emitted + e >= a.max_new) ? 1 : 0;
    a.status[W_STEPS] += 1;
    a.status[W_ACCEPTED] += min(n_match, e);
    a.status[W_REJECTING] += n_match < n_cand ? 1 : 0;
    a.status[W_NMATCH] = n_match;
    a.state[1] += e;   // key-range end
    a.state[2] += e;   // cache slot of the next step's first row
    a.state[3] += e;   // its position
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int afk_lookup_draft(const int* ids, int ids_cap, int* status, const int* state, int k, int ngram, int max_new, const int* eos, int n_eos, int* cand,
                                int64_t* rows, int* pos, int* krange, const void* emb, int64_t ld_emb, int vocab, int H, void* x_out, int64_t ldx, void* stream) {
    AFK_REQUIRE(ids && status && state && cand && rows && pos && krange, "afk_lookup_draft: null pointer (ids, status, state, cand, rows, pos, krange)");
    AFK_REQUIRE(k >= 1 && k <= AFK_LOOKUP_MAX_K && ngram >= 1 && ngram <= AFK_LOOKUP_MAX_NGRAM && max_new >= 1 && ids_cap >= 1,
                "afk_lookup_draft: k = %d, ngram = %d, max_new = %d, ids_cap = %d (1 <= k <= %d, 1 <= ngram <= %d, max_new >= 1, ids_cap >= 1)", k, ngram, max_new,
                ids_cap, AFK_LOOKUP_MAX_K, AFK_LOOKUP_MAX_NGRAM);
    AFK_REQUIRE(n_eos >= 0 && (eos || !n_eos), "afk_lookup_draft: eos list of %d ids%s", n_eos, n_eos > 0 ? " with a null pointer" : " (n_eos >= 0)");
    if (x_out) {
        AFK_REQUIRE(emb && vocab >= 1 && H > 0 && H % 8 == 0 && ld_emb % 8 == 0 && ld_emb >= H && ldx % 8 == 0 && ldx >= H && (uintptr_t)emb % 16 == 0 &&
                        (uintptr_t)x_out % 16 == 0,
                    "afk_lookup_draft: the embedding gather needs emb, vocab >= 1, H %% 8 == 0 and 16-byte rows (ld_emb, ldx multiples of 8, >= H)");
    }
    DraftArgs a = {ids, ids_cap, status, state, k, ngram, max_new, eos, n_eos, cand, (long long*)rows, pos, krange, (const bf16*)emb, ld_emb, vocab, H,
                   (bf16*)x_out, ldx};
    hipLaunchKernelGGL(lookup_draft_kernel, dim3(1), dim3(DRAFT_NT), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_lookup_draft");
    return AFK_OK;
}

extern "C" int afk_lookup_accept(const float* logits, int64_t ld_logits, int V, int M, const int* cand, int* ids, int ids_cap, int64_t* tokens_out, int max_new,
                                 int* status, int* state, const int* eos, int n_eos, int* sel, float* ws, void* stream) {
    AFK_REQUIRE(logits && cand && ids && status && state && sel && ws, "afk_lookup_accept: null pointer (logits, cand, ids, status, state, sel, ws)");
    AFK_REQUIRE(M >= 2 && M <= AFK_LOOKUP_MAX_K + 1 && V >= 1 && V <= AFK_SAMPLE_MAX_V && ld_logits >= V && max_new >= 1 && ids_cap >= 1,
                "afk_lookup_accept: M = %d, V = %d, ld_logits = %lld, max_new = %d (2 <= M <= %d, 1 <= V <= %d, ld_logits >= V, max_new >= 1)", M, V,
                (long long)ld_logits, max_new, AFK_LOOKUP_MAX_K + 1, AFK_SAMPLE_MAX_V);
    AFK_REQUIRE(n_eos >= 0 && (eos || !n_eos), "afk_lookup_accept: eos list of %d ids%s", n_eos, n_eos > 0 ? " with a null pointer" : " (n_eos >= 0)");
    float* part_val = ws;
    int* part_idx = (int*)ws + (AFK_LOOKUP_MAX_K + 1) * AFK_LOOKUP_PARTS;
    const int vec = V % 4 == 0 && ld_logits % 4 == 0 && (uintptr_t)logits % 16 == 0;
    hipLaunchKernelGGL(lookup_argmax_kernel, dim3(AFK_LOOKUP_PARTS, (unsigned)M), dim3(ARG_NT), 0, ST, logits, ld_logits, V, vec, (const int*)status, part_val, part_idx);
    AcceptArgs a = {M, cand, ids, ids_cap, (long long*)tokens_out, max_new, status, state, eos, n_eos, sel, part_val, part_idx};
    hipLaunchKernelGGL(lookup_accept_kernel, dim3(1), dim3(64), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_lookup_accept");
    return AFK_OK;
}
