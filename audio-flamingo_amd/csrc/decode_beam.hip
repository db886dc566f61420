// Beam search on the device for the decode step (generate(num_beams > 1)): what GenerationMixin._beam_search decides on the host after every token -
// _get_top_k_continuations, _update_finished_beams, _get_running_beams_for_next_iteration, _check_early_stop_heuristic and
// _beam_search_has_unfinished_sequences (transformers/generation/utils.py) - as ONE call with no host state, so the step stays capturable, and the
// move of the KV cache by beam parentage as a second one.  The contracts are in include/afk.h.
//
// afk_beam_step is two launches.
//   beam_candidates_kernel   one 1024-thread block per (row, beam): the beam's fp32 log-softmax plus its running score, and its own top `keep` of the V
//                            continuations - the top `keep` of the row's nb * V lie within the union of the per-beam top `keep`.  The log-sum-exp is an
//                            INTEGER sum of round(exp(z - max) * 2^40) (the masses of csrc/decode_sample.hip): no order in it, so an eager and a replayed
//                            step give the same bits.  The `keep`-th largest score comes from an MSB-first radix selection in 11 / 11 / 10-bit passes over
//                            an LDS histogram of counts, never from a sort; where its class of equal scores is larger than what is still needed, a second
//                            selection over the ids of that class takes the lowest ones (the tie rule: lower flat index j * V + token first).
//   beam_merge_kernel        one block per row: ranks the nb * keep candidates (score descending, flat index ascending), then does the step's bookkeeping
//                            on at most 64 candidates and 16 slots in LDS.  The block that arrives last (a counter in the workspace, left at zero) folds
//                            the rows' flags into status = {t, open}.
// Sequences are never gathered in place: a running beam is its back-pointer record bp[t][row][beam] = {token, parent beam}, written once per step and never
// again; a hypothesis that enters a finished slot is materialised there by walking the records back from its parent (t loads).  The finished slots are
// permuted by the merge: their scalars go through registers (every old value is read before a barrier, written behind it), their token rows do not move at
// all - position k of the ranking names its row through fin_slot, and a hypothesis that enters takes the row of one that left.
#include "common.h"
#include "../../include/afk.h"

namespace {

typedef unsigned long long u64;
constexpr int NT = 1024, NW = NT / 64;
constexpr int NBINS = 2048;                    // bins of an 11-bit pass (the last pass has 1024)
constexpr float MASS_ONE = 1099511627776.f;    // 2^40
constexpr float GATE = -1.0e9f;                // the reference's "never" score
constexpr int MAX_NB = AFK_BEAM_MAX_BEAMS, MAX_KEEP = AFK_BEAM_MAX_KEEP;

struct BeamArgs {
    const float* logits; int64_t ld; int B, nb, V, max_new, keep; const int* step_base; int step_off; const int* eos; int n_eos; int es_true;
    const float* div; const float* hdiv; float* run_score; float* fin_score; int* fin_len; int* fin_done; int* fin_slot; int* fin_seq; int* can_improve;
    int* bp; long long* next_token; int* src; int* status; int* ws;
};
// workspace (int32 words): [0] arrival counter, [1 .. 1 + 2B) the rows' {can_improve, every slot filled}, then the candidates' scores and tokens
__host__ __device__ inline int64_t ws_flags_at() { return 1; }
__host__ __device__ inline int64_t ws_score_at(int B) { return 1 + 2 * (int64_t)B; }
__host__ __device__ inline int64_t ws_tok_at(int B, int nb, int keep) { return ws_score_at(B) + (int64_t)B * nb * keep; }
__host__ __device__ inline int64_t ws_words(int B, int nb, int keep) { return ws_tok_at(B, nb, keep) + (int64_t)B * nb * keep; }

// order-preserving key: a < b  <=>  key(a) < key(b)
__device__ __forceinline__ uint32_t key_of(float z) {
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float clean(float x) { return x == x ? x : -INFINITY; }   // NaN counts as -inf, as in the sampler
// accumulated log-probability of a continuation: log_softmax in fp32, then the fp32 add of the beam's running score (the -1e9 of a dead beam absorbs the row)
__device__ __forceinline__ float score_of(float z, float zmax, float lsum, float rs, bool dead_row) {
    float s = ((z - zmax) - lsum) + rs;
    if (dead_row || !(s == s)) s = -INFINITY;
    if (s == 0.f) s = 0.f;   // -0 and +0 are one class
    return s;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive scan over the block's threads in thread order.  Begins with a barrier behind the caller's reads of wtot, ends with every thread holding its value.
__device__ __forceinline__ int block_scan_incl(int v, int* wtot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    __syncthreads();
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) base += i < w ? wtot[i] : 0;
    return v + base;
}
// MSB-first radix selection, descending: among the ids i < V for which keyf(i, key) holds, the key T of the need-th largest, i.e.
// count(key > T) < need <= count(key >= T); gt = count(key > T), eq = count(key == T).  The caller guarantees need <= the number of such ids (a selection that
// finds no bin answers bin 0 with gt = eq = 0: nothing is indexed by it).  Everything returned is block-uniform.  Ends with a barrier.
template <typename KF>
__device__ __forceinline__ uint32_t select_desc(int V, int need, KF&& keyf, int* hist, int* wtot, int* sel, int& gt, int& eq) {
    const int t = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    int rem = need;
    gt = 0, eq = 0;
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, nbins = pass == 2 ? 1024 : 2048;
        for (int i = t; i < NBINS; i += NT) hist[i] = 0;
        if (t == 0) sel[0] = 0, sel[1] = 0, sel[2] = 0;
        __syncthreads();
#pragma unroll 4
        for (int i = t; i < V; i += NT) {
            uint32_t k;
            if (keyf(i, k) && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & (uint32_t)(nbins - 1)], 1);
        }
        __syncthreads();
        const int per = nbins >> 10;   // bins per thread, walked from the top
        const int a0 = hist[nbins - 1 - t * per], a1 = per == 2 ? hist[nbins - 2 - t * per] : 0;
        const int incl = block_scan_incl(a0 + a1, wtot), excl = incl - (a0 + a1);
        if (excl < rem && rem <= incl) {   // one thread
            const int j = rem <= excl + a0 ? 0 : 1;
            sel[0] = nbins - 1 - (t * per + j);
            sel[1] = excl + (j ? a0 : 0);
            sel[2] = j ? a1 : a0;
        }
        __syncthreads();
        prefix |= (uint32_t)sel[0] << shift;
        mask |= (uint32_t)(nbins - 1) << shift;
        gt += sel[1];
        rem -= sel[1];
        eq = sel[2];
        __syncthreads();
    }
    return prefix;
}

// t of this launch, or -1 when the launch must not write: t outside [0, max_new), or the call is closed (status[1] == 0)
__device__ __forceinline__ int live_step(const BeamArgs& a) {
    const int t = (a.step_base ? *a.step_base : 0) + a.step_off;
    if (t < 0 || t >= a.max_new || a.status[1] == 0) return -1;
    return t;
}

__global__ __launch_bounds__(NT) void beam_candidates_kernel(BeamArgs a) {
    __shared__ int hist[NBINS];
    __shared__ int wtot[NW];
    __shared__ u64 wsum[NW];
    __shared__ float wmax[NW];
    __shared__ int sel[4];
    const int t = threadIdx.x, r = blockIdx.x;   // r = row * nb + beam
    if (live_step(a) < 0) return;                // block-uniform
    const float* __restrict__ row = a.logits + (int64_t)r * a.ld;
    const int V = a.V;
    const float rs = a.run_score[r];
    float m = -INFINITY;
#pragma unroll 8
    for (int i = t; i < V; i += NT) m = fmaxf(m, clean(row[i]));
    const float zmax = block_max<NW>(m, wmax);
    const bool dead_row = !(zmax > -INFINITY && zmax < INFINITY);   // no finite maximum: torch's log_softmax answers NaN everywhere, which counts as -inf
    u64 mass = 0;
#pragma unroll 8
    for (int i = t; i < V; i += NT) {
        const float e = dead_row ? 0.f : expf(clean(row[i]) - zmax);
        const u64 q = __float2ull_rn(e * MASS_ONE);
        mass += (e > 0.f && q == 0) ? 1 : q;
    }
    mass = wave_sum_u64(mass);
    if ((t & 63) == 0) wsum[t >> 6] = mass;
    __syncthreads();
    u64 total = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) total += wsum[i];
    const float lsum = dead_row ? 0.f : (float)log((double)total * (1.0 / (double)MASS_ONE));
    auto score = [&](int i) { return score_of(clean(row[i]), zmax, lsum, rs, dead_row); };

    const int kk = a.keep < V ? a.keep : V;   // what this beam hands to the merge
    int gt, eq;
    const uint32_t T = select_desc(V, kk, [&](int i, uint32_t& k) { k = key_of(score(i)); return true; }, hist, wtot, sel, gt, eq);
    uint32_t T2 = 0;   // ids of the threshold class that stay: ~id >= T2
    if (eq > kk - gt) {   // block-uniform: more equal scores at the threshold than places left - the lowest ids of the class
        int gt2, eq2;
        T2 = select_desc(V, kk - gt, [&](int i, uint32_t& k) { k = ~(uint32_t)i; return key_of(score(i)) == T; }, hist, wtot, sel, gt2, eq2);
    }
    if (t == 0) sel[3] = 0;
    __syncthreads();
    float* out_s = (float*)(a.ws + ws_score_at(a.B)) + (int64_t)r * a.keep;
    int* out_i = a.ws + ws_tok_at(a.B, a.nb, a.keep) + (int64_t)r * a.keep;
#pragma unroll 4
    for (int i = t; i < V; i += NT) {
        const float s = score(i);
        const uint32_t k = key_of(s);
        if (k > T || (k == T && ~(uint32_t)i >= T2)) {
            const int p = atomicAdd(&sel[3], 1);   // arrival order: the merge ranks, so the order of this list carries nothing
            if (p < kk) out_s[p] = s, out_i[p] = i;
        }
    }
}

__global__ __launch_bounds__(NT) void beam_merge_kernel(BeamArgs a) {
    __shared__ float sc[MAX_NB * MAX_KEEP];
    __shared__ int fl[MAX_NB * MAX_KEEP];
    __shared__ float cs[MAX_KEEP], rsc[MAX_KEEP], ms[2 * MAX_NB], nf_score[MAX_NB];
    __shared__ int cf[MAX_KEEP], cends[MAX_KEEP], mrank[2 * MAX_NB], nf_done[MAX_NB], newslot[MAX_NB], old_slot[MAX_NB];
    __shared__ float best_run;
    __shared__ int s_last;
    const int tid = threadIdx.x, b = blockIdx.x, nb = a.nb, V = a.V, keep = a.keep;
    const int t = live_step(a);
    if (t < 0) return;   // block-uniform, and the same answer in every block of the launch: status is written only after all of them have read it
    const bool last = t + 1 == a.max_new;
    const int kk = keep < V ? keep : V, N = nb * kk;
    // ---- the row's top `keep` of the nb * kk candidates, in order: score descending, flat index ascending
    if (tid < N) {
        const int j = tid / kk, c = tid - j * kk;
        sc[tid] = ((const float*)(a.ws + ws_score_at(a.B)))[(int64_t)(b * nb + j) * keep + c];
        fl[tid] = j * V + a.ws[ws_tok_at(a.B, nb, keep) + (int64_t)(b * nb + j) * keep + c];
    }
    __syncthreads();
    if (tid < N) {
        const float s = sc[tid];
        const int f = fl[tid];
        int rank = 0;
        for (int m = 0; m < N; ++m) rank += (sc[m] > s || (sc[m] == s && fl[m] < f)) ? 1 : 0;
        if (rank < keep) cs[rank] = s, cf[rank] = f;
    }
    __syncthreads();
    // ---- per candidate: does it end, and its score as a running beam
    const int ci = a.can_improve[b];
    float my_fin_score = 0.f;
    int my_fin_len = 0, my_fin_done = 0, my_fin_slot = 0;
    if (tid < keep) {
        const int tok = cf[tid] % V;
        bool ends = last;
        for (int e = 0; e < a.n_eos; ++e) ends |= a.eos[e] == tok;
        cends[tid] = ends ? 1 : 0;
        rsc[tid] = ends ? cs[tid] + GATE : cs[tid];
    }
    if (tid < nb) {   // the finished slots' scalars go through registers: read here, written behind the barriers below
        my_fin_score = a.fin_score[b * nb + tid], my_fin_len = a.fin_len[b * nb + tid], my_fin_done = a.fin_done[b * nb + tid];
        my_fin_slot = min(max(a.fin_slot[b * nb + tid], 0), nb - 1);   // state from the caller: never an index outside fin_seq
        nf_done[tid] = my_fin_done;   // for `full` below
        old_slot[tid] = my_fin_slot;
    }
    __syncthreads();
    // ---- finished slots: the nb old ones and the top nb candidates, by score / div[t]
    if (tid < 2 * nb) {
        float s;
        if (tid < nb) {
            s = my_fin_score;
        } else {
            const int c = tid - nb;
            bool full = a.es_true != 0;
            for (int k = 0; k < nb; ++k) full = full && nf_done[k] != 0;
            s = cs[c] * (1.0f / a.div[t]);
            if (full || !ci || !cends[c]) s += GATE;
        }
        ms[tid] = s == s ? s : -INFINITY;   // the ranking below needs a total order
    }
    __syncthreads();
    if (tid < 2 * nb) {
        const float s = ms[tid];
        int rank = 0;
        for (int m = 0; m < 2 * nb; ++m) rank += (ms[m] > s || (ms[m] == s && m < tid)) ? 1 : 0;
        mrank[tid] = rank;
    }
    __syncthreads();
    if (tid == 0) {   // a hypothesis that enters takes the token row of one that leaves (as many leave as enter)
        int c = nb;
        for (int k = 0; k < nb; ++k) {
            if (mrank[k] < nb) continue;
            while (mrank[c] >= nb) ++c;
            newslot[mrank[c]] = old_slot[k];
            ++c;
        }
    }
    __syncthreads();
    if (tid < 2 * nb && mrank[tid] < nb) {
        const int q = mrank[tid], at = b * nb + q;
        if (tid < nb) {
            a.fin_score[at] = my_fin_score, a.fin_len[at] = my_fin_len, a.fin_done[at] = my_fin_done, a.fin_slot[at] = my_fin_slot;
            nf_score[q] = my_fin_score, nf_done[q] = my_fin_done;
        } else {
            const int c = tid - nb, slot = newslot[q];
            a.fin_score[at] = ms[tid], a.fin_len[at] = t + 1, a.fin_done[at] = cends[c], a.fin_slot[at] = slot;
            nf_score[q] = ms[tid], nf_done[q] = cends[c];
            int* seq = a.fin_seq + (int64_t)(b * nb + slot) * a.max_new;   // nobody else reads or writes this row in this launch
            seq[t] = cf[c] % V;
            int p = cf[c] / V;
            for (int u = t - 1; u >= 0; --u) {   // records of earlier launches
                const int2 e = ((const int2*)a.bp)[((int64_t)u * a.B + b) * nb + p];
                seq[u] = e.x;
                p = min(max(e.y, 0), nb - 1);
            }
        }
    }
    // ---- running beams: the best nb candidates that do not end
    if (tid < keep) {
        const float s = rsc[tid];
        int rank = 0;
        for (int m = 0; m < keep; ++m) rank += (rsc[m] > s || (rsc[m] == s && m < tid)) ? 1 : 0;
        if (rank < nb) {
            const int at = b * nb + rank, tok = cf[tid] % V, parent = cf[tid] / V;
            a.run_score[at] = s;
            ((int2*)a.bp)[((int64_t)t * a.B + b) * nb + rank] = make_int2(tok, parent);
            a.next_token[at] = tok;
            a.src[at] = b * nb + parent;
            if (rank == 0) best_run = s;
        }
    }
    __syncthreads();
    // ---- can a running beam still beat the worst finished hypothesis?  Then the rows' flags -> status, by the block that arrives last
    if (tid == 0) {
        bool all_done = true;
        float minfin = INFINITY;
        for (int k = 0; k < nb; ++k) all_done = all_done && nf_done[k] != 0, minfin = fminf(minfin, nf_score[k]);
        int ci_new = ci;
        if (!last) {
            const float best = best_run * (1.0f / a.hdiv[t]);
            bool any = false;
            for (int k = 0; k < nb; ++k) any = any || best > (nf_done[k] ? minfin : GATE);
            ci_new = (ci && any) ? 1 : 0;
            a.can_improve[b] = ci_new;
        }
        int* flags = a.ws + ws_flags_at();
        __hip_atomic_store(&flags[2 * b], ci_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&flags[2 * b + 1], all_done ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();   // this block's stores (src included: the barrier above is behind them) before its arrival
        s_last = __hip_atomic_fetch_add(&a.ws[0], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == a.B - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    __shared__ int s_open;
    if (tid == 0) {
        const int* flags = a.ws + ws_flags_at();
        bool any_ci = false, all_rows_done = true;
        for (int r = 0; r < a.B; ++r) {
            any_ci = any_ci || __hip_atomic_load(&flags[2 * r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
            all_rows_done = all_rows_done && __hip_atomic_load(&flags[2 * r + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        }
        s_open = (!last && any_ci && !(a.es_true && all_rows_done)) ? 1 : 0;   // 0: where the host loop breaks
        __hip_atomic_store(&a.ws[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the counter is left at zero
    }
    __syncthreads();
    if (!s_open)   // the host loop breaks in front of the cache move: every beam keeps its own rows
        for (int r = tid; r < a.B * nb; r += NT) a.src[r] = r;
    __threadfence();
    __syncthreads();
    if (tid == 0) a.status[0] = t, a.status[1] = s_open;
}

// ------------------------------------------------------------------------------------------------ the cache move
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;   // 16 bytes as one register quad
struct ReorderArgs {
    bf16* kc; bf16* vt; int L, B, nb, Smax, spad, nk, S0, max_new; const int* src; const int* cur;
};
// the row's parents as beam indices inside its own group, clamped into it; true when the row moves nothing
__device__ __forceinline__ bool load_parents(const ReorderArgs& a, int b, int* par) {
    bool ident = true;
#pragma unroll
    for (int j = 0; j < MAX_NB; ++j) {
        int p = j;
        if (j < a.nb) {
            p = a.src[b * a.nb + j] - b * a.nb;
            p = p < 0 ? 0 : p >= a.nb ? a.nb - 1 : p;
        }
        par[j] = p;
        ident = ident && p == j;
    }
    return ident;
}
// last slot that moves: *cur, clamped to the slots the call may have written
__device__ __forceinline__ int last_slot(const ReorderArgs& a) {
    const int c = *a.cur, hi = a.S0 + a.max_new - 1;
    return c < hi ? c : hi;
}
// Kc [L][B * nb][Smax][nk]: a thread owns one 16-byte chunk of one (layer, row, slot) across the nb beams
__global__ __launch_bounds__(256) void beam_reorder_k_kernel(ReorderArgs a) {
    const int cps = a.nk / 8;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)a.L * a.B * a.max_new * cps;
    if (id >= total) return;
    const int c = (int)(id % cps);
    const int so = (int)((id / cps) % a.max_new);
    const int b = (int)((id / ((int64_t)cps * a.max_new)) % a.B);
    const int l = (int)(id / ((int64_t)cps * a.max_new * a.B));
    const int s = a.S0 + so;
    if (s > last_slot(a)) return;
    int par[MAX_NB];
    if (load_parents(a, b, par)) return;
    u32x4* base = (u32x4*)(a.kc + (((int64_t)l * a.B * a.nb + (int64_t)b * a.nb) * a.Smax + s) * a.nk) + c;
    const int64_t bs = (int64_t)a.Smax * a.nk / 8;   // beam stride in 16-byte units
    u32x4 v[MAX_NB];
#pragma unroll
    for (int j = 0; j < MAX_NB; ++j)
        if (j < a.nb) v[j] = base[par[j] * bs];
#pragma unroll
    for (int j = 0; j < MAX_NB; ++j)
        if (j < a.nb) base[j * bs] = v[j];
}
// Vt [L][B * nb][nk = Hkv * D][spad], the slot innermost: a thread owns one aligned run of 8 slots of one (layer, row, line) across the nb beams; a run that
// lies inside the tail moves as 16 bytes, one that crosses an end of it slot by slot
__global__ __launch_bounds__(256) void beam_reorder_v_kernel(ReorderArgs a) {
    const int c0 = a.S0 / 8, nch = (a.S0 + a.max_new - 1) / 8 - c0 + 1;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)a.L * a.B * a.nk * nch;
    if (id >= total) return;
    const int c = c0 + (int)(id % nch);
    const int line = (int)((id / nch) % a.nk);
    const int b = (int)((id / ((int64_t)nch * a.nk)) % a.B);
    const int l = (int)(id / ((int64_t)nch * a.nk * a.B));
    const int hi = last_slot(a);
    const int s0 = c * 8 > a.S0 ? c * 8 : a.S0, s1 = c * 8 + 7 < hi ? c * 8 + 7 : hi;   // slots [s0, s1] of this run move
    if (s0 > s1) return;
    int par[MAX_NB];
    if (load_parents(a, b, par)) return;
    bf16* base = a.vt + (((int64_t)l * a.B * a.nb + (int64_t)b * a.nb) * a.nk + line) * a.spad;
    const int64_t bs = (int64_t)a.nk * a.spad;   // beam stride in elements
    if (s0 == c * 8 && s1 == c * 8 + 7) {
        u32x4 v[MAX_NB];
#pragma unroll
        for (int j = 0; j < MAX_NB; ++j)
            if (j < a.nb) v[j] = *(const u32x4*)(base + par[j] * bs + c * 8);
#pragma unroll
        for (int j = 0; j < MAX_NB; ++j)
            if (j < a.nb) *(u32x4*)(base + j * bs + c * 8) = v[j];
        return;
    }
    for (int s = s0; s <= s1; ++s) {
        unsigned short v[MAX_NB];
#pragma unroll
        for (int j = 0; j < MAX_NB; ++j)
            if (j < a.nb) v[j] = *(const unsigned short*)(base + par[j] * bs + s);
#pragma unroll
        for (int j = 0; j < MAX_NB; ++j)
            if (j < a.nb) *(unsigned short*)(base + j * bs + s) = v[j];
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t afk_beam_step_workspace_ints(int B, int nb, int n_eos) {
    if (B < 1 || nb < 2 || nb > MAX_NB || n_eos < 0 || ((int64_t)n_eos + 1) * nb > MAX_KEEP) return -1;
    return ws_words(B, nb, (n_eos + 1) * nb);
}

extern "C" int afk_beam_step(const float* logits, int64_t ld_logits, int B, int nb, int V, int max_new, const int* step_base, int step_off, const int* eos,
                             int n_eos, int early_stopping, const float* div, const float* hdiv, float* run_score, float* fin_score, int* fin_len,
                             int* fin_done, int* fin_slot, int* fin_seq, int* can_improve, int* bp, int64_t* next_token, int* src, int* status, int* ws,
                             int64_t ws_ints, void* stream) {
    AFK_REQUIRE(logits && div && hdiv && run_score && fin_score && fin_len && fin_done && fin_slot && fin_seq && can_improve && bp && next_token && src &&
                    status && ws,
                "afk_beam_step: null pointer (logits, div, hdiv, the state, next_token, src, status, ws)");
    AFK_REQUIRE(B >= 1 && V >= 1 && max_new >= 1 && ld_logits >= V, "afk_beam_step: unsupported shape (B >= 1, V >= 1, max_new >= 1, ld_logits >= V)");
    AFK_REQUIRE(((uintptr_t)bp & 7) == 0, "afk_beam_step: bp must be 8-byte aligned");
    AFK_REQUIRE(nb >= 2 && nb <= MAX_NB, "afk_beam_step: %d beams (2 <= nb <= %d)", nb, MAX_NB);
    AFK_REQUIRE(n_eos >= 0 && (eos || !n_eos), "afk_beam_step: eos list of %d ids%s", n_eos, n_eos > 0 ? " with a null pointer" : " (n_eos >= 0)");
    const int64_t keep = ((int64_t)n_eos + 1) * nb;
    AFK_REQUIRE(keep <= MAX_KEEP, "afk_beam_step: keep = (n_eos + 1) * nb = %lld candidates (keep <= %d)", (long long)keep, MAX_KEEP);
    AFK_REQUIRE((int64_t)nb * V >= keep && (int64_t)nb * V < (1ll << 31), "afk_beam_step: nb * V = %lld continuations for keep = %lld (keep <= nb * V < 2^31)",
                (long long)nb * V, (long long)keep);
    AFK_REQUIRE((int64_t)B * nb <= 65535 && (int64_t)max_new * B * nb < (1ll << 30), "afk_beam_step: %d x %d beams over %d steps is beyond the launch's index range",
                B, nb, max_new);
    AFK_REQUIRE(ws_ints >= ws_words(B, nb, (int)keep), "afk_beam_step: workspace of %lld words (needs %lld: afk_beam_step_workspace_ints)", (long long)ws_ints,
                (long long)ws_words(B, nb, (int)keep));
    BeamArgs a = {logits, ld_logits, B, nb, V, max_new, (int)keep, step_base, step_off, eos, n_eos, early_stopping == 1, div, hdiv, run_score, fin_score,
                  fin_len, fin_done, fin_slot, fin_seq, can_improve, bp, (long long*)next_token, src, status, ws};
    hipLaunchKernelGGL(beam_candidates_kernel, dim3(B * nb), dim3(NT), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_beam_step (candidates)");
    hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(NT), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_beam_step (merge)");
    return AFK_OK;
}

extern "C" int afk_beam_reorder_cache(void* kcache, void* vtcache, int L, int B, int nb, int Smax, int spad, int Hkv, int D, int S0, int max_new,
                                      const int* src, const int* cur, void* stream) {
    AFK_REQUIRE(kcache && vtcache && src && cur, "afk_beam_reorder_cache: null pointer (kcache, vtcache, src, cur)");
    AFK_REQUIRE(L >= 1 && B >= 1 && Hkv >= 1 && D >= 1 && S0 >= 0 && max_new >= 1, "afk_beam_reorder_cache: unsupported shape (L, B, Hkv, D, max_new >= 1, S0 >= 0)");
    AFK_REQUIRE(nb >= 2 && nb <= MAX_NB, "afk_beam_reorder_cache: %d beams (2 <= nb <= %d)", nb, MAX_NB);
    const int64_t nk = (int64_t)Hkv * D;
    AFK_REQUIRE(nk % 8 == 0 && nk <= (1 << 20), "afk_beam_reorder_cache: Hkv * D = %lld (16-byte chunks: a multiple of 8)", (long long)nk);
    AFK_REQUIRE((int64_t)S0 + max_new <= Smax && Smax <= spad && spad % 8 == 0,
                "afk_beam_reorder_cache: S0 + max_new = %d + %d slots in a cache of %d, pitch %d (S0 + max_new <= Smax <= spad, spad %% 8 == 0)", S0, max_new, Smax, spad);
    AFK_REQUIRE(((uintptr_t)kcache & 15) == 0 && ((uintptr_t)vtcache & 15) == 0, "afk_beam_reorder_cache: the caches must be 16-byte aligned");
    ReorderArgs a = {(bf16*)kcache, (bf16*)vtcache, L, B, nb, Smax, spad, (int)nk, S0, max_new, src, cur};
    const int64_t nk_threads = (int64_t)L * B * max_new * (nk / 8);
    const int64_t nv_threads = (int64_t)L * B * nk * ((S0 + max_new - 1) / 8 - S0 / 8 + 1);
    AFK_REQUIRE(afk_cdiv(nk_threads, 256) < (1ll << 31) && afk_cdiv(nv_threads, 256) < (1ll << 31), "afk_beam_reorder_cache: the tail is beyond one launch's grid");
    hipLaunchKernelGGL(beam_reorder_k_kernel, dim3((unsigned)afk_cdiv(nk_threads, 256)), dim3(256), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_beam_reorder_cache (K)");
    hipLaunchKernelGGL(beam_reorder_v_kernel, dim3((unsigned)afk_cdiv(nv_threads, 256)), dim3(256), 0, ST, a);
    AFK_LAUNCH_CHECK("afk_beam_reorder_cache (V)");
    return AFK_OK;
}
