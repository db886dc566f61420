// Classifier-free guidance inside the decode step (generate(guidance_scale=...); UnbatchedClassifierFreeGuidanceLogitsProcessor,
// transformers/generation/logits_process.py:2224-2339): afk_decode_cfg folds the fp32 logits of a conditional and an unconditional row into
// out = scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond).  Two plain launches over 8 KB column chunks, so a step of 1 .. 8 rows
// spreads over the CUs: the first leaves (max, sum of exp) per chunk and row, the second folds those pairs in one fixed order and writes its chunk of the row.
// Enqueue-only, allocation-free, capturable; no counters, no atomics: the bits depend on the inputs and the shape alone.
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr int CFG_NT = 256, CFG_NW = CFG_NT / 64;
constexpr int CFG_VPT = 2;                          // 16-byte vectors per thread and row
constexpr int CFG_CHUNK = CFG_NT * CFG_VPT * 4;     // columns per block: 2 048 (75 chunks for the AF3 vocabulary of 152 064)

// the thread's 4 * CFG_VPT values of the chunk at column c0 of `row` (V columns): vector j covers the columns c0 + 4 * (j * CFG_NT + tid) .. + 3.  A 16-byte load
// where the vector lies inside the row and the address allows it, word loads otherwise - the SAME columns either way, so the alignment of a row never
// changes which thread holds which value.  A NaN counts as -inf (the sampler's and afk_beam_step's convention), and so does a column >= V, which is not read.
__device__ __forceinline__ void cfg_load(const float* __restrict__ row, int64_t c0, int V, int tid, float (&x)[4 * CFG_VPT]) {
    const bool vec = (((uintptr_t)(row + c0)) & 15u) == 0;   // block-uniform
#pragma unroll
    for (int j = 0; j < CFG_VPT; ++j) {
        const int64_t c = c0 + 4 * (int64_t)(j * CFG_NT + tid);
        if (vec && c + 3 < V) {
            const f32x4 v = *(const f32x4*)(row + c);
            x[4 * j] = v[0], x[4 * j + 1] = v[1], x[4 * j + 2] = v[2], x[4 * j + 3] = v[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * j + e] = (c + e < V) ? row[c + e] : -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) x[4 * j + e] = (x[4 * j + e] != x[4 * j + e]) ? -INFINITY : x[4 * j + e];
    }
}

// ws[((b * 2 + r) * nchunk + k) * 2 + {0, 1}] = {max, sum of expf(x - max)} of chunk k of row b of cond (r = 0) / uncond (r = 1); a chunk with no entry above
// -inf leaves {-inf, 0}.  grid (nchunk, B).  One fixed order of additions: the thread's values in column order, the wave's xor tree, the waves in ascending order.
__global__ __launch_bounds__(CFG_NT) void decode_cfg_partials_kernel(const float* __restrict__ cond, int64_t ld_c, const float* __restrict__ uncond, int64_t ld_u,
                                                                     int V, int nchunk, float* __restrict__ ws) {
    __shared__ float scratch[CFG_NW];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t c0 = (int64_t)k * CFG_CHUNK;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float* __restrict__ row = r == 0 ? cond + (int64_t)b * ld_c : uncond + (int64_t)b * ld_u;
        float x[4 * CFG_VPT];
        cfg_load(row, c0, V, tid, x);
        float m = x[0];
#pragma unroll
        for (int e = 1; e < 4 * CFG_VPT; ++e) m = fmaxf(m, x[e]);
        m = block_max<CFG_NW>(m, scratch);
        float s = 0.f;
        if (m != -INFINITY) {   // block-uniform.  m == +inf: inf - inf is NaN and the row's sum with it, as in log_softmax
#pragma unroll
            for (int e = 0; e < 4 * CFG_VPT; ++e) s += expf(x[e] - m);
        }
        s = block_sum<CFG_NW>(s, scratch);
        if (tid == 0) {
            float* w = ws + (((int64_t)b * 2 + r) * nchunk + k) * 2;
            w[0] = m, w[1] = s;
        }
    }
}

// the row's {max, log of the sum} from the chunk pairs, by the whole block and in one fixed order: thread i takes the chunks i, i + CFG_NT, ... in ascending order,
// then the wave's xor tree, then the waves in ascending order (75 pairs at the AF3 vocabulary: one per thread).  A first form in which every thread folded all
// pairs itself, a serial loop of 150 expf, measured 37 us per call at B = 1 where this one measures 9 (profiles/cfg_decode.md).
__device__ __forceinline__ void cfg_fold(const float* __restrict__ w, int nchunk, int tid, float* scratch, float& M, float& logS) {
    float m = -INFINITY;
    for (int k = tid; k < nchunk; k += CFG_NT) m = fmaxf(m, w[2 * k]);
    M = block_max<CFG_NW>(m, scratch);
    float s = 0.f;
    for (int k = tid; k < nchunk; k += CFG_NT) {
        const float mk = w[2 * k];
        if (mk != -INFINITY) s += w[2 * k + 1] * expf(mk - M);
    }
    logS = logf(block_sum<CFG_NW>(s, scratch));
}

// out[b][c] = scale * (lc - lu) + lu with lc = (cond[b][c] - Mc) - log Sc and lu likewise: log_softmax as torch evaluates it, then the reference's expression with
// every product and sum rounded on its own (no fused multiply-add).  grid (nchunk, B); a block reads and writes its own chunk only, so out may be cond.
__global__ __launch_bounds__(CFG_NT) void decode_cfg_apply_kernel(const float* cond, int64_t ld_c, const float* __restrict__ uncond, int64_t ld_u, float scale,
                                                                  float* out, int64_t ld_o, int V, int nchunk, const float* __restrict__ ws) {
    __shared__ float scratch[CFG_NW];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t c0 = (int64_t)k * CFG_CHUNK;
    float Mc, Lc, Mu, Lu;
    cfg_fold(ws + ((int64_t)b * 2 + 0) * nchunk * 2, nchunk, tid, scratch, Mc, Lc);
    cfg_fold(ws + ((int64_t)b * 2 + 1) * nchunk * 2, nchunk, tid, scratch, Mu, Lu);
    float xc[4 * CFG_VPT], xu[4 * CFG_VPT];
    cfg_load(cond + (int64_t)b * ld_c, c0, V, tid, xc);
    cfg_load(uncond + (int64_t)b * ld_u, c0, V, tid, xu);
    float* o = out + (int64_t)b * ld_o;
    const bool vec = (((uintptr_t)(o + c0)) & 15u) == 0;   // block-uniform
#pragma unroll
    for (int j = 0; j < CFG_VPT; ++j) {
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lc = __fsub_rn(__fsub_rn(xc[4 * j + e], Mc), Lc), lu = __fsub_rn(__fsub_rn(xu[4 * j + e], Mu), Lu);
            y[e] = __fadd_rn(__fmul_rn(scale, __fsub_rn(lc, lu)), lu);
        }
        const int64_t c = c0 + 4 * (int64_t)(j * CFG_NT + tid);
        if (vec && c + 3 < V) {
            *(f32x4*)(o + c) = y;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < V) o[c + e] = y[e];
        }
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t afk_decode_cfg_workspace_floats(int B, int V) {
    if (B < 1 || V < 1) return 0;
    return (int64_t)B * 4 * afk_cdiv(V, CFG_CHUNK);
}

extern "C" int afk_decode_cfg(const float* cond, int64_t ld_c, const float* uncond, int64_t ld_u, float scale, float* out, int64_t ld_o, int B, int V, float* ws,
                              int64_t ws_floats, void* stream) {
    AFK_REQUIRE(cond && uncond && out && ws, "afk_decode_cfg: null pointer (cond, uncond, out, ws)");
    AFK_REQUIRE(B >= 1 && B <= 65535, "afk_decode_cfg: B = %d rows (1 <= B <= 65535)", B);
    AFK_REQUIRE(V >= 1, "afk_decode_cfg: V = %d columns (V >= 1)", V);
    AFK_REQUIRE(ld_c >= V && ld_u >= V && ld_o >= V, "afk_decode_cfg: leading dimension below V (ld_c %lld, ld_u %lld, ld_o %lld, V %d)", (long long)ld_c,
                (long long)ld_u, (long long)ld_o, V);
    AFK_REQUIRE(ws_floats >= afk_decode_cfg_workspace_floats(B, V), "afk_decode_cfg: workspace of %lld floats, needs %lld (afk_decode_cfg_workspace_floats)",
                (long long)ws_floats, (long long)afk_decode_cfg_workspace_floats(B, V));
    const int nchunk = (int)afk_cdiv(V, CFG_CHUNK);
    hipLaunchKernelGGL(decode_cfg_partials_kernel, dim3(nchunk, B), dim3(CFG_NT), 0, ST, cond, ld_c, uncond, ld_u, V, nchunk, ws);
    AFK_LAUNCH_CHECK("afk_decode_cfg (partials)");
    hipLaunchKernelGGL(decode_cfg_apply_kernel, dim3(nchunk, B), dim3(CFG_NT), 0, ST, cond, ld_c, uncond, ld_u, scale, out, ld_o, V, nchunk, ws);
    AFK_LAUNCH_CHECK("afk_decode_cfg (apply)");
    return AFK_OK;
}
