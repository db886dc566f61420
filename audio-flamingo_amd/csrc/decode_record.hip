// Keeping the per-step rows of generate(return_dict_in_generate=True): afk_decode_record copies the fp32 logits (or processed scores) of the step into slot t of
// a [n_steps][B][V] buffer from inside the captured decode step; afk_transition_scores is GenerationMixin.compute_transition_scores
// (transformers/generation/utils.py:1433-1555, the branch without beam_indices) on such a buffer.  Both are enqueue-only, allocation-free and capturable.
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr int REC_NT = 256;
constexpr int REC_VPT = 4;                       // 16-byte vectors per thread
constexpr int REC_VPB = REC_NT * REC_VPT;        // vectors per block: a 16 KB column chunk (38 chunks for the 608 KB row of the AF3 vocabulary)

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// dst[t][b][0 .. V) = src[b][0 .. V) as 32-bit words (NaN payloads, -0 and the infinities survive).  grid (column chunks, B).  The row is cut at the first
// 16-byte boundary of the DESTINATION: a scalar head in front of it, 16-byte stores behind it (16-byte loads where the source shares the alignment, four word
// loads per store where it does not), a scalar tail of up to three words.  t outside [0, n_steps) writes nothing.
__global__ __launch_bounds__(REC_NT) void decode_record_kernel(const unsigned int* __restrict__ src, int64_t ld_src, int V, unsigned int* __restrict__ dst,
                                                               int64_t step_stride, int64_t ld_dst, int n_steps, const int* __restrict__ step_base, int step_off) {
    const int t = (step_base ? *step_base : 0) + step_off;
    if (t < 0 || t >= n_steps) return;   // block-uniform
    const int b = blockIdx.y, tid = threadIdx.x;
    const unsigned int* __restrict__ s = src + (int64_t)b * ld_src;
    unsigned int* __restrict__ d = dst + (int64_t)t * step_stride + (int64_t)b * ld_dst;
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2));   // words in front of the destination's first 16-byte boundary
    const int nvec = (V - head) >> 2, tail0 = head + 4 * nvec;                            // [head, tail0) in vectors, [tail0, V) scalar
    const bool src_vec = (((uintptr_t)(s + head)) & 15u) == 0;
    const unsigned int* __restrict__ sb = s + head;
    unsigned int* __restrict__ db = d + head;
    const int v0 = blockIdx.x * REC_VPB;
    u32x4 r[REC_VPT];
    if (src_vec) {
#pragma unroll
        for (int j = 0; j < REC_VPT; ++j) {
            const int v = v0 + j * REC_NT + tid;
            if (v < nvec) r[j] = *(const u32x4*)(sb + 4 * (int64_t)v);
        }
    } else {
#pragma unroll
        for (int j = 0; j < REC_VPT; ++j) {
            const int v = v0 + j * REC_NT + tid;
            if (v < nvec) {
                const unsigned int* p = sb + 4 * (int64_t)v;
                r[j] = u32x4{p[0], p[1], p[2], p[3]};
            }
        }
    }
#pragma unroll
    for (int j = 0; j < REC_VPT; ++j) {
        const int v = v0 + j * REC_NT + tid;
        if (v < nvec) *(u32x4*)(db + 4 * (int64_t)v) = r[j];
    }
    if (blockIdx.x == 0) {   // head and tail: at most three words each
        if (tid < head) d[tid] = s[tid];
        const int i = tail0 + tid - 64;
        if (tid >= 64 && i < V) d[i] = s[i];
    }
}

constexpr int TS_NT = 1024, TS_NW = TS_NT / 64, TS_LU = 4;

// out[b][t] = scores[t][b][tok] - (normalize ? logsumexp(scores[t][b][:]) : 0).  One block of TS_NT threads per (t, b) row, whatever the shape: thread i takes the
// ids i, i + TS_NT, ... in ascending order, then the wave's xor tree, then the waves in ascending order - one fixed order of additions per V.
__global__ __launch_bounds__(TS_NT) void transition_scores_kernel(const float* __restrict__ scores, int64_t step_stride, int64_t ld, int V,
                                                                  const long long* __restrict__ tokens, int64_t ld_tokens, int normalize,
                                                                  float* __restrict__ out, int64_t ld_out) {
    __shared__ float scratch[TS_NW];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* __restrict__ row = scores + (int64_t)t * step_stride + (int64_t)b * ld;
    float lse = 0.f;
    if (normalize) {
        float m = -INFINITY;
        for (int i0 = tid; i0 < V; i0 += TS_LU * TS_NT) {
            float x[TS_LU];
#pragma unroll
            for (int u = 0; u < TS_LU; ++u) x[u] = (i0 + u * TS_NT < V) ? row[i0 + u * TS_NT] : -INFINITY;
#pragma unroll
            for (int u = 0; u < TS_LU; ++u) m = fmaxf(m, x[u]);
        }
        m = block_max<TS_NW>(m, scratch);
        float acc = 0.f;
        for (int i0 = tid; i0 < V; i0 += TS_LU * TS_NT) {
            float x[TS_LU];
#pragma unroll
            for (int u = 0; u < TS_LU; ++u) x[u] = (i0 + u * TS_NT < V) ? row[i0 + u * TS_NT] : -INFINITY;
#pragma unroll
            for (int u = 0; u < TS_LU; ++u)
                if (i0 + u * TS_NT < V) acc += expf(x[u] - m);   // -inf - finite max: 0; no finite entry: -inf - -inf = NaN, as log_softmax; a NaN entry stays one
        }
        acc = block_sum<TS_NW>(acc, scratch);
        lse = m + logf(acc);
    }
    if (tid == 0) {
        const long long tok = tokens[(int64_t)b * ld_tokens + t];
        float r = NAN;   // an id outside the vocabulary is refused on the host; never read out of bounds here
        if (tok >= 0 && tok < V) r = row[tok] - lse;
        out[(int64_t)b * ld_out + t] = r;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int afk_decode_record(const float* src, int64_t ld_src, int B, int V, float* dst, int64_t step_stride, int64_t ld_dst, int n_steps, const int* step_base,
                                 int step_off, void* stream) {
    AFK_REQUIRE(src && dst, "afk_decode_record: null pointer (src, dst)");
    AFK_REQUIRE(B >= 1 && B <= 65535 && V >= 1 && n_steps >= 1 && ld_src >= V && ld_dst >= V && step_stride >= (int64_t)(B - 1) * ld_dst + V,
                "afk_decode_record: unsupported shape (1 <= B <= 65535, V >= 1, n_steps >= 1, row strides >= V, step_stride >= (B - 1) * ld_dst + V)");
    AFK_REQUIRE(step_base || (step_off >= 0 && step_off < n_steps), "afk_decode_record: step %d outside the buffer's %d slots", step_off, n_steps);
    const int chunks = (int)afk_cdiv(afk_cdiv(V, 4), REC_VPB);
    hipLaunchKernelGGL(decode_record_kernel, dim3(chunks, B), dim3(REC_NT), 0, ST, (const unsigned int*)src, ld_src, V, (unsigned int*)dst, step_stride, ld_dst, n_steps,
                       step_base, step_off);
    AFK_LAUNCH_CHECK("afk_decode_record");
    return AFK_OK;
}

extern "C" int afk_transition_scores(const float* scores, int64_t step_stride, int64_t ld, int T, int B, int V, const int64_t* tokens, int64_t ld_tokens, int normalize,
                                     float* out, int64_t ld_out, void* stream) {
    AFK_REQUIRE(scores && tokens && out, "afk_transition_scores: null pointer (scores, tokens, out)");
    AFK_REQUIRE(T >= 1 && B >= 1 && B <= 65535 && V >= 1 && ld >= V && ld_tokens >= T && ld_out >= T && step_stride >= 0,
                "afk_transition_scores: unsupported shape (T >= 1, 1 <= B <= 65535, V >= 1, ld >= V, ld_tokens >= T, ld_out >= T)");
    hipLaunchKernelGGL(transition_scores_kernel, dim3(T, B), dim3(TS_NT), 0, ST, scores, step_stride, ld, V, (const long long*)tokens, ld_tokens, normalize, out, ld_out);
    AFK_LAUNCH_CHECK("afk_transition_scores");
    return AFK_OK;
}
