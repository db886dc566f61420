// The stopping rule of the decode step on the device (generate(eos_token_id=[...], stop_strings=...)): what GenerationMixin's loop decides on the host after
// every token - EosTokenCriteria and StopStringCriteria (transformers/generation/stopping_criteria.py), then `next_tokens * unfinished + pad * (1 - unfinished)` -
// as one launch with no host state, so the step stays capturable.  The contract is in include/afk.h.
//
// One block.  A wave takes the rows b = wave, wave + STOP_NW, ...; everything a row's decision reads is either in registers (the token just selected) or was
// written by an EARLIER launch (the older ids, stop_at), so no lane waits for another lane's store.  Inside a row the lanes stride over the eos ids and over the
// (stop string, end-length) pairs of the reference's table; each pair is the reference's cumsum / mask recurrence walked from the newest id backwards.
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr int STOP_NT = 256, STOP_NW = STOP_NT / 64;

struct StopArgs {
    long long* next_token; int B; int* ids; int64_t ld_ids; int S0; int max_new; int* stop_at; int* status; const int* step_base; int step_off;
    const int* eos; int neos; int pad; int feed_pad; const int* table; int rows; int vec; int P; int E; int S; const int* target; int W;
};

__global__ __launch_bounds__(STOP_NT) void decode_stop_kernel(StopArgs a) {
    __shared__ int s_open[STOP_NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = (a.step_base ? *a.step_base : 0) + a.step_off;
    if (t < 0 || t >= a.max_new) return;   // block-uniform: nothing is written, status included
    int open = 0;                          // rows of this wave that are still unfinished behind step t (wave-uniform)
    for (int b = wave; b < a.B; b += STOP_NW) {
        int* row = a.ids + (int64_t)b * a.ld_ids;
        const int at = a.stop_at[b];
        long long tok64 = a.next_token[b];
        if (at < t) tok64 = a.pad;         // finished earlier: the reference emits (and feeds) pad_token_id
        const int tok = (int)tok64;
        if (lane == 0) {
            row[a.S0 + t] = tok;
            if (at < t && a.feed_pad) a.next_token[b] = a.pad;
        }
        if (at < t) continue;
        // ---- EosTokenCriteria: the token is one of the eos ids
        bool hit = false;
        for (int i = lane; i < a.neos; i += 64) hit |= a.eos[i] == tok;
        // ---- StopStringCriteria.__call__ on the last min(W, n) ids, newest first
        if (a.S > 0) {
            const int64_t n = (int64_t)a.S0 + t + 1;
            const int m = (int)(n < a.W ? n : a.W);
            const int dummy = a.rows - 1;   // ids beyond the table (and, defensively, negative ones) take the dummy row
            const int* r0 = a.table + (int64_t)((tok < 0 || tok > dummy) ? dummy : tok) * a.vec;
            for (int pe = lane; pe < a.S * a.E; pe += 64) {
                const int s = pe / a.E;
                int c = r0[a.P * a.S + pe];   // = P * S + E * s + e
                if (c <= 0) continue;
                int best = c;
                for (int j = 1; j < m; ++j) {
                    const int id = row[a.S0 + t - j];   // written by an earlier launch, or prompt
                    const int* rj = a.table + (int64_t)((id < 0 || id > dummy) ? dummy : id) * a.vec;
                    bool ok = false;
                    for (int k = 0; k < a.P; ++k) ok |= rj[a.P * s + k] == c;
                    if (!ok) break;
                    c += rj[a.vec - 1];
                    best = max(best, c);
                }
                hit |= best >= a.target[s];
            }
        }
        if (__any(hit)) {
            if (lane == 0) a.stop_at[b] = t;
        } else if (at > t) {
            ++open;   // at == t without a hit cannot happen on the same data; a replay of step t finds its own hit again
        }
    }
    if (!a.status) return;
    if (lane == 0) s_open[wave] = open;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < STOP_NW; ++w) total += s_open[w];
        a.status[0] = t;
        a.status[1] = total;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int afk_decode_stop(int64_t* next_token, int B, int* ids, int64_t ld_ids, int S0, int max_new, int* stop_at, int* status, const int* step_base,
                               int step_off, const int* eos, int n_eos, int pad, int feed_pad, const int* table, int rows, int vec, int P, int E, int S,
                               const int* target_lens, int W, void* stream) {
    AFK_REQUIRE(next_token && ids && stop_at, "afk_decode_stop: null pointer (next_token, ids, stop_at)");
    AFK_REQUIRE(B >= 1 && S0 >= 0 && max_new >= 1, "afk_decode_stop: unsupported shape (B >= 1, S0 >= 0, max_new >= 1)");
    AFK_REQUIRE((int64_t)S0 + max_new <= ld_ids, "afk_decode_stop: S0 + max_new = %d + %d ids in rows of %lld (S0 + max_new <= ld_ids)", S0, max_new,
                (long long)ld_ids);
    AFK_REQUIRE(n_eos >= 0 && (eos || !n_eos), "afk_decode_stop: eos list of %d ids%s", n_eos, n_eos > 0 ? " with a null pointer" : " (n_eos >= 0)");
    AFK_REQUIRE(S >= 0, "afk_decode_stop: %d stop strings (S >= 0; 0 switches them off)", S);
    if (S > 0) {
        AFK_REQUIRE(table && target_lens, "afk_decode_stop: stop strings with a null table (table, target_lens)");
        AFK_REQUIRE(rows >= 1 && P >= 1 && E >= 1 && W >= 1 && (int64_t)S * E <= (1 << 20) && (int64_t)vec == (int64_t)S * ((int64_t)P + E) + 1,
                    "afk_decode_stop: table of %d rows x %d for S = %d, P = %d, E = %d, W = %d (rows, P, E, W >= 1, vec == S * (P + E) + 1)", rows, vec, S, P, E, W);
    }
    StopArgs a = {(long long*)next_token, B, ids, ld_ids, S0, max_new, stop_at, status, step_base, step_off, eos, n_eos, pad, feed_pad, table, rows, vec, P, E,
                  S, target_lens, W};
    hipLaunchKernelGGL(decode_stop_kernel, dim3(1), dim3(STOP_NT), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_decode_stop");
    return AFK_OK;
}
