// Token sampling on the device for the decode step (generate(do_sample=True)): temperature -> top-k -> top-p -> min_p -> typical_p -> epsilon_cutoff ->
// eta_cutoff -> draw, one launch, no host state - the step can be captured into a HIP graph like the greedy one.  Oracle: TemperatureLogitsWarper /
// TopKLogitsWarper / TopPLogitsWarper / MinPLogitsWarper / TypicalLogitsWarper / EpsilonLogitsWarper / EtaLogitsWarper
// (transformers/generation/logits_process.py) and the multinomial draw of GenerationMixin._sample (transformers/generation/utils.py).
//
// One 1024-thread block per row of fp32 logits (the 608 KB row of the AF3 vocabulary stays in L2 across the passes).  Floats map to order-preserving
// 32-bit keys; thresholds come from MSB-first radix selection in 11 / 11 / 10-bit passes over LDS histograms, never from a sort:
//   top-k   histogram of COUNTS,  walked from the top:    the key of the min(top_k, V)-th largest value (ties at the threshold all stay, as `logits < kth` keeps them)
//   top-p   histogram of MASSES over the K-set, walked from the bottom: the smallest key whose inclusive cumulative mass exceeds (1 - top_p) x the K-set's mass
//           (the reference's ascending cumsum including the token itself; a class of equal values stays or goes as a whole)
//   min_p / epsilon / eta   a probability floor over the current set S is a floor in z: z >= zmax + log(floor x Z_S), folded into the top-k / top-p threshold key -
//           no pass of their own beyond the statistics of S (mass, sum of mass x (zmax - z), largest z: one pass, integer and max reductions)
//   typical_p   -log r_i - H = (zmax - z_i) - E with E = sum_S r_j (zmax - z_j): log Z cancels, no per-token log.  Keys of d = |(zmax - z) - E|, histogram of
//           MASSES over S walked from the bottom: the smallest d whose inclusive cumulative mass reaches typical_p x mass(S).  The kept set becomes a band in z
//           that may exclude the row maximum - kernel instantiation TYP, whose membership test in_set() carries the d key next to the threshold key
//   draw    masses of the kept set in token-id order: per-granule sums, one block scan, one wave walks the granule that holds u x total
// Every mass is the 64-bit fixed-point integer round(exp(z - max) * 2^40), at least 1 where the exponential is positive: integer sums do not depend on the
// order of the LDS atomics or on the launch geometry, so the token is a pure function of (logits, parameters, u).  The quantisation is 2^-40 of the largest
// term per token (1.4e-7 of the total over 152 064 tokens), far below fp32 exp's own error.  The entropy term is the integer sum of
// round(exp(z - max) * (max - z) * 2^40) (each term below 0.37 * 2^40: no overflow up to AFK_SAMPLE_MAX_V), order-free in the same way.
// The kernel is instantiated three times: <TYP = false, FLT = false> with none of the four filters active - the code and the passes from before they existed -,
// <false, true> with block-uniform branches outside the per-logit loops around the floors' statistics passes, and <true, true> for typical_p < 1.
#include "common.h"
#include "../../include/afk.h"

namespace {

typedef unsigned long long u64;
constexpr int NT = 1024, NW = NT / 64;
constexpr int NB = 2048;        // bins of an 11-bit pass (the last pass has 1024)
constexpr int NG_MAX = 4096;    // granule sums of the draw held in LDS: four per thread
constexpr float MASS_ONE = 1099511627776.f;   // 2^40

struct SampleArgs {
    const float* logits; int64_t ld; int V; float T; int top_k; float top_p; const float* u; uint32_t key0, key1; const int* step_base; int step_off;
    long long* next_token; float* probs; int64_t ld_probs; int* kept; long long* tokens_out; int tok_off; int* state; const bf16* emb; int64_t ld_emb; int H;
    bf16* x_out;
    float min_p, typical_p, eps, eta;   // as passed; off: min_p <= 0, typical_p >= 1, eps / eta outside (0, 1)
    float* scores; int64_t scores_ss, ld_scores; int n_steps;   // afk_decode_sample_scored: the warped row of token t goes to slot t of [n_steps][B][V] (null: not wanted)
};
struct Sel { int bin; u64 excl, total, target; };

// z = logits / T (fp32 division as the warper's `scores / temperature`; T == 1: untouched); NaN counts as -inf, -0 as +0 (one class with +0)
__device__ __forceinline__ float zval(float x, float T, bool div) {
    float z = div ? x / T : x;
    if (!(z == z)) z = -INFINITY;
    if (z == 0.f) z = 0.f;
    return z;
}
// order-preserving key: a < b  <=>  key(a) < key(b)
__device__ __forceinline__ uint32_t key_of(float z) {
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u64 mass_of(float z, float zmax) {
    const float e = expf(z - zmax);
    const u64 m = __float2ull_rn(e * MASS_ONE);
    return (e > 0.f && m == 0) ? 1 : m;   // a kept token with a positive probability can be drawn (u = 0 answers the lowest kept id)
}
// the entropy term of a token: exp(z - zmax) * (zmax - z) in the fixed point of the masses
__device__ __forceinline__ u64 gapmass_of(float z, float zmax) {
    const float g = zmax - z;
    return __float2ull_rn(expf(z - zmax) * g * MASS_ONE);
}
// key of the typical-decoding distance d = |-log r - H| = |(zmax - z) - E|, E = the mass-weighted mean of (zmax - z) over the set
__device__ __forceinline__ uint32_t dkey_of(float z, float zmax, float E) { return key_of(fabsf((zmax - z) - E)); }
// THE membership test of the kept set, one expression for every pass that asks: at or above the threshold key, finite, and (TYP) inside the typical band
template <bool TYP>
__device__ __forceinline__ bool in_set(float z, uint32_t thr, float zmax, float E, uint32_t dthr) {
    bool k = key_of(z) >= thr && z > -INFINITY;
    if (TYP) k = k && dkey_of(z, zmax, E) <= dthr;
    return k;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block-wide integer sum (all threads get it).  Begins and ends with a barrier, so wtot can be reused at once.
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* wtot) {
    v = wave_sum_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) r += wtot[i];
    __syncthreads();
    return r;
}
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {   // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}
// inclusive scan over the block's threads in thread order; total = the block's sum
__device__ __forceinline__ u64 block_scan_incl(u64 v, u64* wtot, u64& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_scan_u64(v, lane);
    __syncthreads();
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const u64 x = wtot[i];
        if (i < w) base += x;
        tot += x;
    }
    total = tot;
    return v + base;
}
// the first bin, walking h[0 .. nb) upwards (or downwards: desc), whose inclusive running sum exceeds `target` (use_frac: target = frac x the sum of all bins);
// sel = {bin, the running sum in front of it, the sum of all bins, target}.  nb = 1024 or 2048.  Ends with a barrier.
template <typename HT>
__device__ __forceinline__ void select_bin(const HT* h, int nb, bool desc, bool use_frac, double frac, u64 target, u64* wtot, Sel* sel) {
    const int t = threadIdx.x, per = nb >> 10;
    u64 a[2] = {0, 0};
    for (int j = 0; j < per; ++j) {
        const int p = t * per + j;
        a[j] = h[desc ? nb - 1 - p : p];
    }
    if (t == 0) { sel->bin = desc ? 0 : nb - 1; sel->excl = 0; sel->total = 0; sel->target = 0; }   // never left unset (a bin is always found: see the callers)
    const u64 local = a[0] + a[1];
    u64 total;
    const u64 incl = block_scan_incl(local, wtot, total), excl = incl - local;
    if (use_frac) {
        target = (u64)(frac * (double)total);
        if (total && target >= total) target = total - 1;
    }
    if (excl <= target && target < incl) {   // one thread
        const int j = (target < excl + a[0]) ? 0 : 1;
        const int p = t * per + j;
        sel->bin = desc ? nb - 1 - p : p;
        sel->excl = excl + (j ? a[0] : 0);
        sel->total = total;
        sel->target = target;
    }
    __syncthreads();
}

// f(i, logits[i]) for the ids i = t, t + 1024, ... of a row, eight loads in flight per thread (one load per round trip: 197 / 297 us per launch for top-k /
// top-k + top-p at V = 152 064, eight: 183 / 259 - the passes are bound by the one CU's vector ALU, profiles/decode_sampling.md)
constexpr int LU = 8;
template <typename F>
__device__ __forceinline__ void for_each_logit(const float* __restrict__ row, int V, int t, F&& f) {
    int base = 0;
    for (; base + LU * NT <= V; base += LU * NT) {
        float x[LU];
#pragma unroll
        for (int u = 0; u < LU; ++u) x[u] = row[base + u * NT + t];
#pragma unroll
        for (int u = 0; u < LU; ++u) f(base + u * NT + t, x[u]);
    }
    float x[LU];
#pragma unroll
    for (int u = 0; u < LU; ++u) {
        const int i = base + u * NT + t;
        x[u] = i < V ? row[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < LU; ++u) {
        const int i = base + u * NT + t;
        if (i < V) f(i, x[u]);
    }
}

// statistics of the current set (BAND: the typical band is part of it): its mass, its entropy term sum mass x (zmax - z), its largest z.  Integer sums
// and a max: no order in them.  Ends with a barrier on wtot; wmax is written behind one.
template <bool BAND>
__device__ __forceinline__ void set_stats(const float* __restrict__ row, int V, int t, float T, bool div, float zmax, uint32_t thr, float E, uint32_t dthr,
                                          u64* wtot, float* wmax, u64& total, u64& gap, float& ztop) {
    u64 m = 0, g = 0;
    float zt = -INFINITY;
    for_each_logit(row, V, t, [&](int, float x) {
        const float z = zval(x, T, div);
        if (in_set<BAND>(z, thr, zmax, E, dthr)) {
            m += mass_of(z, zmax);
            g += gapmass_of(z, zmax);
            zt = fmaxf(zt, z);
        }
    });
    total = block_sum_u64(m, wtot);
    gap = block_sum_u64(g, wtot);
    ztop = block_max<NW>(zt, wmax);
}
// the threshold key of a probability floor over a set of mass `total` (2^40 = the row maximum's own mass): softmax_S(z)_i >= floor <=> z_i >= zmax +
// log(floor x total / 2^40); the class of the set's largest z (ztop) stays whatever the floor
__device__ __forceinline__ uint32_t floor_key(float zmax, double floor, u64 total, float ztop) {
    float zt = (float)((double)zmax + log(floor * ((double)total * (1.0 / (double)MASS_ONE))));
    if (zt == 0.f) zt = 0.f;
    return min(key_of(zt), key_of(ztop));
}

// Philox4x32-10 (Salmon et al., SC'11), word 0 of the output block
__device__ __forceinline__ uint32_t philox4x32_10_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// TYP: typical_p < 1 - the kept set is a band in z, not a threshold.  FLT: one of the four filters is active; <false, false> holds none of their code
template <bool TYP, bool FLT>
__global__ __launch_bounds__(NT) void decode_sample_kernel(SampleArgs a) {
    __shared__ u64 hmass[NB];
    __shared__ unsigned int hcnt[NB];
    __shared__ u64 gsum[NG_MAX];
    __shared__ u64 wtot[NW];
    __shared__ float wmax_s[NW];
    __shared__ int winf_s[NW], wcnt_s[NW];
    __shared__ Sel sel;
    __shared__ int s_tok, s_step;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.x, V = a.V;
    const float* __restrict__ row = a.logits + (int64_t)b * a.ld;
    const float T = a.T;
    const bool div = T != 1.f;
    const int kk = (a.top_k > 0 && a.top_k < V) ? a.top_k : 0;   // 0: every token is in the K-set
    const bool use_p = a.top_p < 1.f;
    if (t == 0) s_step = (a.step_base ? *a.step_base : 0) + a.step_off;   // read before the bookkeeping below advances the state it may live in

    // ---- pass A: row maximum, lowest +inf, and the first count histogram
    for (int i = t; i < NB; i += NT) hcnt[i] = 0;
    __syncthreads();
    float zmax = -INFINITY;
    int iinf = 0x7fffffff;
    for_each_logit(row, V, t, [&](int i, float x) {
        const float z = zval(x, T, div);
        zmax = fmaxf(zmax, z);
        if (z == INFINITY) iinf = min(iinf, i);
        if (kk) atomicAdd(&hcnt[key_of(z) >> 21], 1u);
    });
    zmax = wave_max(zmax);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) iinf = min(iinf, __shfl_xor(iinf, o, 64));
    if (lane == 0) { wmax_s[w] = zmax; winf_s[w] = iinf; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NW; ++i) { zmax = fmaxf(zmax, wmax_s[i]); iinf = min(iinf, winf_s[i]); }
    const int mode = iinf != 0x7fffffff ? 1 : (zmax == -INFINITY ? 2 : 0);   // 1: a +inf wins (lowest index); 2: no finite logit -> 0; both as torch.argmax

    int tok = mode == 1 ? iinf : 0, kept_n = mode == 1 ? 1 : 0;
    uint32_t thr = 0, dthr = 0xffffffffu;   // the kept set: in_set<TYP>(z, thr, zmax, E, dthr)
    float inv_tot = 0.f, E = 0.f;
    if (mode == 0) {
        // ---- top-k: key of the kk-th largest value
        uint32_t kth = 0;
        if (kk) {
            uint32_t pfx = 0;
            u64 rem = (u64)(kk - 1);
            for (int p = 0; p < 3; ++p) {
                const int sh = p == 0 ? 21 : p == 1 ? 10 : 0, bits = p == 2 ? 10 : 11, nb = 1 << bits;
                if (p > 0) {
                    for (int i = t; i < nb; i += NT) hcnt[i] = 0;
                    __syncthreads();
                    for_each_logit(row, V, t, [&](int, float x) {
                        const uint32_t key = key_of(zval(x, T, div));
                        if ((key >> (sh + bits)) == pfx) atomicAdd(&hcnt[(key >> sh) & (nb - 1)], 1u);
                    });
                    __syncthreads();
                }
                select_bin(hcnt, nb, true, false, 0.0, rem, wtot, &sel);   // the bins hold at least rem + 1 elements: V >= kk, then the chosen bin's count
                pfx = (pfx << bits) | (uint32_t)sel.bin;
                rem -= sel.excl;
            }
            kth = pfx;
        }
        thr = kth;
        // ---- top-p over the K-set: the smallest key whose inclusive cumulative mass exceeds (1 - top_p) of the K-set's mass
        if (use_p) {
            uint32_t pfx = 0;
            u64 rem = 0;
            for (int p = 0; p < 3; ++p) {
                const int sh = p == 0 ? 21 : p == 1 ? 10 : 0, bits = p == 2 ? 10 : 11, nb = 1 << bits;
                for (int i = t; i < nb; i += NT) hmass[i] = 0;
                __syncthreads();
                for_each_logit(row, V, t, [&](int, float x) {
                    const float z = zval(x, T, div);
                    const uint32_t key = key_of(z);
                    if (key >= kth && (p == 0 || (key >> (sh + bits)) == pfx)) atomicAdd(&hmass[(key >> sh) & (nb - 1)], mass_of(z, zmax));
                });
                __syncthreads();
                // the maximum is in the K-set with mass 2^40, and (1 - top_p) < 1: the target is below the total in every pass
                select_bin(hmass, nb, false, p == 0, 1.0 - (double)a.top_p, rem, wtot, &sel);
                pfx = (pfx << bits) | (uint32_t)sel.bin;
                rem = sel.target - sel.excl;
            }
            thr = pfx;   // >= kth: only K-set keys were counted
        }
        // ---- min_p over the P-set, whose maximum is the row's: exp(z - zmax) >= min_p as a floor in z (min_p == 1: the ties with the maximum stay)
        if (FLT && a.min_p > 0.f) thr = max(thr, floor_key(zmax, (double)a.min_p, (u64)1 << 40, zmax));
        // ---- typical_p: the smallest distance d* whose inclusive cumulative mass, tokens taken by ascending d, reaches typical_p of the set's mass
        if (TYP) {
            u64 total, gap;
            float ztop;
            set_stats<false>(row, V, t, T, div, zmax, thr, 0.f, 0u, wtot, wmax_s, total, gap, ztop);
            E = (float)((double)gap / (double)total);   // total >= 2^40: the row maximum is in the set
            uint32_t pfx = 0;
            u64 rem = 0;
            for (int p = 0; p < 3; ++p) {
                const int sh = p == 0 ? 21 : p == 1 ? 10 : 0, bits = p == 2 ? 10 : 11, nb = 1 << bits;
                for (int i = t; i < nb; i += NT) hmass[i] = 0;
                __syncthreads();
                for_each_logit(row, V, t, [&](int, float x) {
                    const float z = zval(x, T, div);
                    const uint32_t dk = dkey_of(z, zmax, E);
                    if (in_set<false>(z, thr, zmax, E, dthr) && (p == 0 || (dk >> (sh + bits)) == pfx)) atomicAdd(&hmass[(dk >> sh) & (nb - 1)], mass_of(z, zmax));
                });
                __syncthreads();
                // typical_p < 1: the target is below the total in pass 0, and inside the chosen bin's mass afterwards
                select_bin(hmass, nb, false, p == 0, (double)a.typical_p, rem, wtot, &sel);
                pfx = (pfx << bits) | (uint32_t)sel.bin;
                rem = sel.target - sel.excl;
            }
            dthr = pfx;   // the band holds the token that reached the target: its mass is positive
        }
        // ---- epsilon_cutoff, then eta_cutoff with eta = min(eps, sqrt(eps) exp(-H)): probability floors over the set as it stands in front of each
        for (int f = 0; FLT && f < 2; ++f) {
            const float eps = f == 0 ? a.eps : a.eta;
            if (!(eps > 0.f && eps < 1.f)) continue;
            u64 total, gap;
            float ztop;
            set_stats<TYP>(row, V, t, T, div, zmax, thr, E, dthr, wtot, wmax_s, total, gap, ztop);
            double floor = (double)eps;
            if (f == 1) {   // H = log Z + sum r (zmax - z), Z = total / 2^40
                const double Z = (double)total * (1.0 / (double)MASS_ONE), H = log(Z) + (double)gap / (double)total;
                floor = fmin(floor, sqrt(floor) * exp(-H));
            }
            thr = max(thr, floor_key(zmax, floor, total, ztop));
        }
        // ---- draw: masses of the kept set in token-id order
        float u;
        if (a.u) {
            u = a.u[b];
        } else {
            u = (float)(philox4x32_10_w0((uint32_t)s_step, (uint32_t)b, 0u, 0u, a.key0, a.key1) >> 8) * 5.9604644775390625e-8f;
        }
        if (!(u >= 0.f)) u = 0.f;
        if (u >= 1.f) u = 1.f - 5.9604644775390625e-8f;
        const int m = (V + 64 * NG_MAX - 1) / (64 * NG_MAX), gran = 64 * m, ngran = (V + gran - 1) / gran;   // granule = 64 m consecutive ids, at most NG_MAX of them
        int cnt = 0;
        for (int g0 = w; g0 < ngran; g0 += NW * LU) {   // LU granules of a wave per round trip (granules g0, g0 + 16, ...)
            u64 s[LU];
#pragma unroll
            for (int q = 0; q < LU; ++q) s[q] = 0;
            for (int j = 0; j < m; ++j) {
                float x[LU];
#pragma unroll
                for (int q = 0; q < LU; ++q) {
                    const int g = g0 + q * NW, i = g * gran + j * 64 + lane;
                    x[q] = (g < ngran && i < V) ? row[i] : -INFINITY;   // -inf is never kept
                }
#pragma unroll
                for (int q = 0; q < LU; ++q) {
                    const float z = zval(x[q], T, div);
                    if (in_set<TYP>(z, thr, zmax, E, dthr)) { s[q] += mass_of(z, zmax); ++cnt; }
                }
            }
#pragma unroll
            for (int q = 0; q < LU; ++q) {
                const u64 sum = wave_sum_u64(s[q]);
                if (lane == 0 && g0 + q * NW < ngran) gsum[g0 + q * NW] = sum;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) wcnt_s[w] = cnt;
        __syncthreads();
        if (t == 0) { sel.bin = 0; sel.excl = 0; }   // the barriers of the scan below order this before the finder's write
        kept_n = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) kept_n += wcnt_s[i];
        u64 a4[4], local = 0, total;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = 4 * t + j;
            a4[j] = g < ngran ? gsum[g] : 0;
            local += a4[j];
        }
        const u64 incl = block_scan_incl(local, wtot, total), excl = incl - local;
        u64 target = (u64)((double)u * (double)total);   // total >= 1 (every filter leaves a token of positive mass), u < 1
        if (target >= total) target = total - 1;
        if (excl <= target && target < incl) {
            u64 e = excl;
            for (int j = 0; j < 4; ++j) {
                if (target < e + a4[j]) { sel.bin = 4 * t + j; sel.excl = e; break; }
                e += a4[j];
            }
        }
        __syncthreads();
        if (w == 0) {   // one wave walks the granule that holds the target
            const int g = sel.bin;
            u64 base = sel.excl;
            int found = -1;
            for (int j = 0; j < m && found < 0; ++j) {
                const int i = g * gran + j * 64 + lane;
                u64 v = 0;
                if (i < V) {
                    const float z = zval(row[i], T, div);
                    if (in_set<TYP>(z, thr, zmax, E, dthr)) v = mass_of(z, zmax);
                }
                const u64 sc = wave_scan_u64(v, lane);
                const u64 hit = __ballot(base + sc > target);
                if (hit) found = g * gran + j * 64 + (int)__ffsll((long long)hit) - 1;
                base += __shfl(sc, 63, 64);
            }
            if (lane == 0) s_tok = found < 0 ? 0 : found;
        }
        __syncthreads();
        tok = s_tok;
        inv_tot = 1.f / (float)((double)total * (1.0 / (double)MASS_ONE));
    }

    // ---- outputs
    if (a.probs) {
        float* pr = a.probs + (int64_t)b * a.ld_probs;
        for_each_logit(row, V, t, [&](int i, float x) {
            float r = 0.f;
            if (mode == 0) {
                const float z = zval(x, T, div);
                if (in_set<TYP>(z, thr, zmax, E, dthr)) r = expf(z - zmax) * inv_tot;
            } else if (mode == 1) {
                r = i == tok ? 1.f : 0.f;
            }
            pr[i] = r;
        });
    }
    if (a.scores && s_step >= 0 && s_step < a.n_steps) {   // what the warper chain leaves in next_token_scores: z on the kept set, -inf elsewhere; s_step was read before the bookkeeping below
        float* sc = a.scores + (int64_t)s_step * a.scores_ss + (int64_t)b * a.ld_scores;
        for_each_logit(row, V, t, [&](int i, float x) {
            float r = -INFINITY;
            if (mode == 0) {
                const float z = zval(x, T, div);
                if (in_set<TYP>(z, thr, zmax, E, dthr)) r = z;
            } else if (mode == 1) {
                if (i == tok) r = zval(x, T, div);   // the +inf that wins; mode 2: no id has a positive probability
            }
            sc[i] = r;
        });
    }
    if (t == 0) {
        a.next_token[b] = tok;
        if (a.kept) a.kept[b] = kept_n;
        if (a.state) {   // the bookkeeping block of decode_select_greedy_kernel (one sequence)
            if (a.tokens_out) a.tokens_out[a.state[2] + a.tok_off] = tok;
            a.state[1] += 1;   // key-range end
            a.state[2] += 1;   // cache slot of the next token
            a.state[3] += 1;   // its position
        }
    }
    if (a.state) {
        const bf16* erow = a.emb + (int64_t)tok * a.ld_emb;
        for (int k = t * 4; k < a.H; k += 4 * NT) *(bf16x4*)(a.x_out + k) = *(const bf16x4*)(erow + k);
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int afk_decode_sample_scored(const float* logits, int64_t ld_logits, int B, int V, float temperature, int top_k, float top_p, float min_p, float typical_p,
                                        float epsilon_cutoff, float eta_cutoff, const float* u, int64_t seed, const int* step_base, int step_off,
                                        int64_t* next_token, float* probs_out, int64_t ld_probs, int* kept_out, int64_t* tokens_out, int tok_off, int* state,
                                        const void* emb, int64_t ld_emb, int H, void* x_out, float* scores_out, int64_t scores_step_stride, int64_t ld_scores,
                                        int n_steps, void* stream) {
    AFK_REQUIRE(logits && next_token, "afk_decode_sample: null pointer (logits, next_token)");
    AFK_REQUIRE(B >= 1 && V >= 1 && V <= AFK_SAMPLE_MAX_V && ld_logits >= V && (!probs_out || ld_probs >= V),
                "afk_decode_sample: unsupported shape (B >= 1, 1 <= V <= %d, row strides >= V)", AFK_SAMPLE_MAX_V);
    AFK_REQUIRE(!scores_out || (n_steps >= 1 && ld_scores >= V && scores_step_stride >= (int64_t)(B - 1) * ld_scores + V),
                "afk_decode_sample: scores_out needs n_steps >= 1, ld_scores >= V and scores_step_stride >= (B - 1) * ld_scores + V");
    AFK_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, "afk_decode_sample: temperature %g (finite, temperature > 0)", (double)temperature);
    AFK_REQUIRE(top_p > 0.f, "afk_decode_sample: top_p %g (top_p > 0; top_p >= 1 switches the filter off)", (double)top_p);
    AFK_REQUIRE(min_p <= 1.f, "afk_decode_sample: min_p %g (min_p <= 1; min_p <= 0 switches the filter off)", (double)min_p);
    AFK_REQUIRE(typical_p > 0.f, "afk_decode_sample: typical_p %g (typical_p > 0; typical_p >= 1 switches the filter off)", (double)typical_p);
    AFK_REQUIRE(epsilon_cutoff == epsilon_cutoff && eta_cutoff == eta_cutoff,
                "afk_decode_sample: epsilon_cutoff %g / eta_cutoff %g (not a number; values outside (0, 1) switch the filters off)", (double)epsilon_cutoff,
                (double)eta_cutoff);
    AFK_REQUIRE(!state || (B == 1 && emb && x_out && H > 0 && H % 4 == 0 && ld_emb % 4 == 0),
                "afk_decode_sample: the bookkeeping block (state) needs B == 1, emb, x_out and H %% 4 == 0");
    AFK_REQUIRE(state || !tokens_out, "afk_decode_sample: tokens_out is indexed by state[2]: null pointer (state)");
    SampleArgs a = {logits, ld_logits, V, temperature, top_k, top_p, u, (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32), step_base, step_off,
                    (long long*)next_token, probs_out, ld_probs, kept_out, (long long*)tokens_out, tok_off, state, (const bf16*)emb, ld_emb, H, (bf16*)x_out,
                    min_p, typical_p, epsilon_cutoff, eta_cutoff, scores_out, scores_step_stride, ld_scores, scores_out ? n_steps : 0};
    const bool floors = min_p > 0.f || (epsilon_cutoff > 0.f && epsilon_cutoff < 1.f) || (eta_cutoff > 0.f && eta_cutoff < 1.f);
    if (typical_p < 1.f) {
        hipLaunchKernelGGL((decode_sample_kernel<true, true>), dim3(B), dim3(NT), 0, ST, a);
    } else if (floors) {
        hipLaunchKernelGGL((decode_sample_kernel<false, true>), dim3(B), dim3(NT), 0, ST, a);
    } else {
        hipLaunchKernelGGL((decode_sample_kernel<false, false>), dim3(B), dim3(NT), 0, ST, a);
    }
    AFK_LAUNCH_CHECK("afk_decode_sample");
    return AFK_OK;
}

extern "C" int afk_decode_sample_filtered(const float* logits, int64_t ld_logits, int B, int V, float temperature, int top_k, float top_p, float min_p, float typical_p,
                                          float epsilon_cutoff, float eta_cutoff, const float* u, int64_t seed, const int* step_base, int step_off,
                                          int64_t* next_token, float* probs_out, int64_t ld_probs, int* kept_out, int64_t* tokens_out, int tok_off, int* state,
                                          const void* emb, int64_t ld_emb, int H, void* x_out, void* stream) {
    return afk_decode_sample_scored(logits, ld_logits, B, V, temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, u, seed, step_base, step_off,
                                    next_token, probs_out, ld_probs, kept_out, tokens_out, tok_off, state, emb, ld_emb, H, x_out, nullptr, 0, 0, 0, stream);
}

extern "C" int afk_decode_sample(const float* logits, int64_t ld_logits, int B, int V, float temperature, int top_k, float top_p, const float* u, int64_t seed,
                                 const int* step_base, int step_off, int64_t* next_token, float* probs_out, int64_t ld_probs, int* kept_out, int64_t* tokens_out,
                                 int tok_off, int* state, const void* emb, int64_t ld_emb, int H, void* x_out, void* stream) {
    return afk_decode_sample_filtered(logits, ld_logits, B, V, temperature, top_k, top_p, 0.f, 1.f, 0.f, 0.f, u, seed, step_base, step_off, next_token, probs_out,
                                      ld_probs, kept_out, tokens_out, tok_off, state, emb, ld_emb, H, x_out, stream);
}
