// Assisted (speculative) decoding on the device (generate(assistant_model=draft, num_assistant_tokens=k)): the two pieces of host work that
// GenerationMixin._assisted_decoding (transformers/generation/utils.py:3562-3830) does around the draft model's steps with an AssistedCandidateGenerator
// (transformers/generation/candidate_generator.py) - handing the draft model the sequence as the target left it, and turning the drafted tokens into the input
// rows of the target's verify forward - as launches with no host state, so that begin -> k draft steps -> stage -> verify forward -> afk_lookup_accept is one
// capturable step.  The contract is in include/afk.h.
//
// Both are a handful of integers and a gather of 16-byte pieces of embedding rows, on the critical path between two weight-streaming launches: one block each,
// nothing to reduce, no atomics, no counters.  What they cost is one round trip to memory per dependent load, so the blocks are sized to have every piece of the
// gather in flight at once - 256 threads cover one row of up to 2 048 columns (begin), 1 024 threads the k + 1 rows of the verify forward (stage: 2 688
// pieces at k = 5 and a hidden size of 3 584) - rather than to fill the machine.
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr int BEGIN_NT = 256, STAGE_NT = 1024;
enum { W_LEN = 0, W_EMITTED = 1, W_DONE = 2, W_NCAND = 3 };

__device__ inline bool is_eos(int tok, const int* eos, int n_eos) {
    for (int i = 0; i < n_eos; ++i)
        if (eos[i] == tok) return true;
    return false;
}

__global__ __launch_bounds__(BEGIN_NT) void assist_begin_kernel(const int* __restrict__ ids, int ids_cap, const int* __restrict__ status,
                                                                const int* __restrict__ state, int* __restrict__ dstate, const bf16* __restrict__ emb,
                                                                int64_t ld_emb, int vocab, int H, bf16* __restrict__ x_out) {
    const int t = threadIdx.x;
    if (t < 4) dstate[t] = state[t];
    const int len = min(max(status[W_LEN], 1), ids_cap);
    const int tok = min(max(ids[len - 1], 0), vocab - 1);
    const bf16* row = emb + (int64_t)tok * ld_emb;
    for (int c = t; c < H / 8; c += BEGIN_NT) *(bf16x8*)(x_out + c * 8) = *(const bf16x8*)(row + c * 8);
}

struct StageArgs {
    const int* ids; int ids_cap; int* status; const int* state; int k; int max_new; const int* eos; int n_eos; const long long* draft; int draft_cap;
    int* cand; long long* rows; int* pos; int* krange; const bf16* emb; int64_t ld_emb; int vocab; int H; bf16* x_out; int64_t ldx;
};

__global__ __launch_bounds__(STAGE_NT) void assist_stage_kernel(StageArgs a) {
    __shared__ int s_tok[AFK_LOOKUP_MAX_K + 1];
    __shared__ int s_ncand;
    const int t = threadIdx.x;
    const int len = min(max(a.status[W_LEN], 1), a.ids_cap);
    const int last = a.ids[len - 1];
    const int budget = a.max_new - a.status[W_EMITTED] - 1;   // a step emits its accepted candidates and one more token
    const bool open = a.status[W_DONE] == 0 && budget > 0;
    const int cur = a.state[2];
    if (t < a.k) s_tok[t + 1] = (int)a.draft[min(max(cur + t, 0), a.draft_cap - 1)];   // drafted token j stands at the cache slot its step appended at
    if (t == 0) s_tok[0] = last;
    __syncthreads();
    if (t == 0) {
        int n = open ? min(a.k, budget) : 0;
        for (int i = 0; i < n; ++i)
            if (is_eos(s_tok[i + 1], a.eos, a.n_eos)) { n = i + 1; break; }   // cut BEHIND the first eos id: the target may confirm it
        s_ncand = n;
        a.status[W_NCAND] = n;
    }
    __syncthreads();
    const int n_cand = s_ncand, M = a.k + 1;
    if (t >= 1 && t < M && t > n_cand) s_tok[t] = last;   // rows behind n_cand run on a valid id; nobody reads their logits (each thread owns its entry)
    __syncthreads();
    if (t < M) {
        if (t >= 1) a.cand[t - 1] = s_tok[t];
        a.rows[t] = s_tok[t];
        a.pos[t] = a.state[3] + t;
        a.krange[2 * t] = a.state[0];
        a.krange[2 * t + 1] = a.state[1] + t;   // row j sees the cache up to its own slot: a staircase over one sequence
    }
    const int pieces = a.H / 8;
    for (int i = t; i < M * pieces; i += STAGE_NT) {
        const int j = i / pieces, c = i % pieces;
        const int tok = min(max(s_tok[j], 0), a.vocab - 1);
        *(bf16x8*)(a.x_out + (int64_t)j * a.ldx + c * 8) = *(const bf16x8*)(a.emb + (int64_t)tok * a.ld_emb + c * 8);
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int afk_assist_begin(const int* ids, int ids_cap, const int* status, const int* state, int* dstate, const void* emb, int64_t ld_emb, int vocab, int H,
                                void* x_out, void* stream) {
    AFK_REQUIRE(ids && status && state && dstate && emb && x_out, "afk_assist_begin: null pointer (ids, status, state, dstate, emb, x_out)");
    AFK_REQUIRE(ids_cap >= 1 && vocab >= 1, "afk_assist_begin: ids_cap = %d, vocab = %d (both >= 1)", ids_cap, vocab);
    AFK_REQUIRE(H > 0 && H % 8 == 0 && ld_emb % 8 == 0 && ld_emb >= H && (uintptr_t)emb % 16 == 0 && (uintptr_t)x_out % 16 == 0,
                "afk_assist_begin: H = %d, ld_emb = %lld: the embedding gather needs H %% 8 == 0 and 16-byte rows (ld_emb a multiple of 8, >= H)", H,
                (long long)ld_emb);
    hipLaunchKernelGGL(assist_begin_kernel, dim3(1), dim3(BEGIN_NT), 0, ST, ids, ids_cap, status, state, dstate, (const bf16*)emb, ld_emb, vocab, H, (bf16*)x_out);
    AFK_LAUNCH_CHECK("afk_assist_begin");
    return AFK_OK;
}

extern "C" int afk_assist_stage(const int* ids, int ids_cap, int* status, const int* state, int k, int max_new, const int* eos, int n_eos, const int64_t* draft,
                                int draft_cap, int* cand, int64_t* rows, int* pos, int* krange, const void* emb, int64_t ld_emb, int vocab, int H, void* x_out,
                                int64_t ldx, void* stream) {
    AFK_REQUIRE(ids && status && state && draft && cand && rows && pos && krange && emb && x_out,
                "afk_assist_stage: null pointer (ids, status, state, draft, cand, rows, pos, krange, emb, x_out)");
    AFK_REQUIRE(k >= 1 && k <= AFK_LOOKUP_MAX_K && max_new >= 1 && ids_cap >= 1 && draft_cap >= 1 && vocab >= 1,
                "afk_assist_stage: k = %d, max_new = %d, ids_cap = %d, draft_cap = %d, vocab = %d (1 <= k <= %d, the others >= 1)", k, max_new, ids_cap, draft_cap,
                vocab, AFK_LOOKUP_MAX_K);
    AFK_REQUIRE(n_eos >= 0 && (eos || !n_eos), "afk_assist_stage: eos list of %d ids%s", n_eos, n_eos > 0 ? " with a null pointer" : " (n_eos >= 0)");
    AFK_REQUIRE(H > 0 && H % 8 == 0 && ld_emb % 8 == 0 && ld_emb >= H && ldx % 8 == 0 && ldx >= H && (uintptr_t)emb % 16 == 0 && (uintptr_t)x_out % 16 == 0,
                "afk_assist_stage: H = %d, ld_emb = %lld, ldx = %lld: the embedding gather needs H %% 8 == 0 and 16-byte rows (ld_emb, ldx multiples of 8, >= H)", H,
                (long long)ld_emb, (long long)ldx);
    StageArgs a = {ids, ids_cap, status, state, k, max_new, eos, n_eos, (const long long*)draft, draft_cap, cand, (long long*)rows, pos, krange,
                   (const bf16*)emb, ld_emb, vocab, H, (bf16*)x_out, ldx};
    hipLaunchKernelGGL(assist_stage_kernel, dim3(1), dim3(STAGE_NT), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_assist_stage");
    return AFK_OK;
}
