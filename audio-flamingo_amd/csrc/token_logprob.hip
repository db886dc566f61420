// Per-token log-probabilities of the lm_head, differentiable (gfx950, HBM-bound).
//
// The second loss-head stage beside ce.hip: where ce_fwd_bwd_kernel turns a logits chunk into d(mean CE)/d(logits) during the forward sweep
// (upstream gradient 1, one shared denominator), these two kernels split the work so that the upstream gradient may differ per row and may depend
// on the log-probabilities themselves (a ratio, a sigmoid of a sequence sum):
//   token_logprob_kernel      ONE sweep over a row of the chunk, no write to it: logp = x[label] - lse, lse, and optionally the entropy
//   token_logprob_bwd_kernel  ONE sweep over the RECOMPUTED chunk with the saved lse: x <- bf16(u * (onehot(label) - exp(x - lse)))
// The forward sweep is pass 1 of ce_fwd_bwd_kernel restated expression for expression: logp is -row_loss of afk_ce_fwd_bwd(write_grad = 0)
// bit for bit (tests/test_token_logprob_gpu.py pins it).  One 256-thread block per row, 16-byte accesses, the V % 8 last columns as a scalar tail.
// Traffic per row: forward 2*V bytes read; backward 2*V read + 2*V written.  No atomics, no counters: both kernels are deterministic.
#include "common.h"
#include "../../include/afk.h"

namespace {

// entropy = -sum p log p on SHIFTED values d = x - m <= 0:  H = log s - t / s,  s = sum e^d,  t = sum e^d d.  A common offset of the row is gone
// before anything is rounded (x and m are bf16 values: d is exact in fp32).  t is carried online beside s: when the running maximum moves from m
// to mx, e^(x - mx) (x - mx) = e^(m - mx) e^(x - m) ((x - m) + (m - mx)), hence t <- e^(m - mx) (t + (m - mx) s).  A -inf logit adds 0 to both.
template <bool ENT>
__global__ __launch_bounds__(256) void token_logprob_kernel(const bf16* __restrict__ logits, int64_t ld, int V,
                                                            const int64_t* __restrict__ labels, float* __restrict__ logp,
                                                            float* __restrict__ lse_out, float* __restrict__ entropy) {
    __shared__ float scratch[8];
    const int64_t row = blockIdx.x;
    const bf16* x = logits + row * ld;
    const int64_t label = labels[row];
    const int tid = threadIdx.x;
    const int nv = V >> 3;
    if (label < 0) {  // ignore_index
        if (tid == 0) {
            logp[row] = 0.f;
            lse_out[row] = 0.f;
            if (ENT) entropy[row] = 0.f;
        }
        return;
    }
    float m = -INFINITY, s = 0.f, t = 0.f;
    for (int v = tid; v < nv; v += 256) {
        const bf16x8 tv = *(const bf16x8*)(x + 8 * v);
        float f[8], mx = m;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            f[e] = (float)tv[e];
            mx = fmaxf(mx, f[e]);
        }
        // nothing finite yet (masked vocabulary: -inf logits): exp(-inf - -inf) is NaN, for the terms and for the rescale; the sums stay 0
        if (mx == -INFINITY) continue;
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += __expf(f[e] - mx);
        if (ENT) {
            float tacc = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = f[e] - mx;
                tacc += (f[e] == -INFINITY) ? 0.f : __expf(d) * d;
            }
            const float dm = m - mx;   // -inf while this thread has seen nothing finite: s = t = 0 and -inf * 0 must not be formed
            t = ((m == -INFINITY) ? 0.f : __expf(dm) * (t + dm * s)) + tacc;
        }
        s = s * __expf(m - mx) + acc;
        m = mx;
    }
    for (int c = nv * 8 + tid; c < V; c += 256) {
        const float f = (float)x[c];
        const float mx = fmaxf(m, f);
        if (mx == -INFINITY) continue;
        if (ENT) {
            const float d = f - mx, dm = m - mx;
            t = ((m == -INFINITY) ? 0.f : __expf(dm) * (t + dm * s)) + ((f == -INFINITY) ? 0.f : __expf(d) * d);
        }
        s = s * __expf(m - mx) + __expf(f - mx);
        m = mx;
    }
    const float gm = block_max<4>(m, scratch);
    if (ENT) {
        const float dm = m - gm;
        t = (m == -INFINITY) ? 0.f : __expf(dm) * (t + dm * s);
    }
    s = (m == -INFINITY) ? 0.f : s * __expf(m - gm);
    const float gs = block_sum<4>(s, scratch);
    const float lse = gm + __logf(gs);
    const float xl = (float)x[label];
    if (tid == 0) {
        logp[row] = xl - lse;
        lse_out[row] = lse;
    }
    if (ENT) {
        const float gt = block_sum<4>(t, scratch);
        if (tid == 0) entropy[row] = __logf(gs) - gt / gs;
    }
}

__global__ __launch_bounds__(256) void token_logprob_bwd_kernel(bf16* __restrict__ logits, int64_t ld, int V,
                                                                const int64_t* __restrict__ labels, const float* __restrict__ lse_in,
                                                                const float* __restrict__ upstream) {
    const int64_t row = blockIdx.x;
    bf16* x = logits + row * ld;
    const int64_t label = labels[row];
    const int tid = threadIdx.x;
    const int nv = V >> 3;
    if (label < 0) {  // ignore_index: zeros whatever the upstream gradient holds (it is not read)
        bf16x8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
        for (int v = tid; v < nv; v += 256) *(bf16x8*)(x + 8 * v) = z;
        for (int c = nv * 8 + tid; c < V; c += 256) x[c] = (bf16)0.f;
        return;
    }
    const float lse = lse_in[row];
    const float u = upstream[row];
    for (int v = tid; v < nv; v += 256) {
        const bf16x8 tv = *(const bf16x8*)(x + 8 * v);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float p = __expf((float)tv[e] - lse);
            const float h = ((int64_t)(8 * v + e) == label) ? 1.f - p : -p;
            o[e] = (bf16)(u * h);
        }
        *(bf16x8*)(x + 8 * v) = o;
    }
    for (int c = nv * 8 + tid; c < V; c += 256) {
        const float p = __expf((float)x[c] - lse);
        const float h = (c == label) ? 1.f - p : -p;
        x[c] = (bf16)(u * h);
    }
}

}  // namespace

extern "C" int afk_token_logprob(const void* logits, int64_t ld, int64_t rows, int V, const int64_t* shift_labels, float* logp, float* lse,
                                 float* entropy, void* stream) {
    AFK_REQUIRE(logits && shift_labels && logp && lse && rows > 0 && V > 0, "afk_token_logprob: bad args");
    AFK_REQUIRE(ld % 8 == 0 && ld >= V && ((uintptr_t)logits % 16 == 0), "afk_token_logprob: logits rows must be 16-byte aligned");
    if (entropy)
        hipLaunchKernelGGL(token_logprob_kernel<true>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)logits, ld, V,
                           shift_labels, logp, lse, entropy);
    else
        hipLaunchKernelGGL(token_logprob_kernel<false>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const bf16*)logits, ld, V,
                           shift_labels, logp, lse, entropy);
    AFK_LAUNCH_CHECK("afk_token_logprob");
    return AFK_OK;
}

extern "C" int afk_token_logprob_bwd(void* logits, int64_t ld, int64_t rows, int V, const int64_t* shift_labels, const float* lse,
                                     const float* upstream, void* stream) {
    AFK_REQUIRE(logits && shift_labels && lse && upstream && rows > 0 && V > 0, "afk_token_logprob_bwd: bad args");
    AFK_REQUIRE(ld % 8 == 0 && ld >= V && ((uintptr_t)logits % 16 == 0), "afk_token_logprob_bwd: logits rows must be 16-byte aligned");
    hipLaunchKernelGGL(token_logprob_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (bf16*)logits, ld, V, shift_labels,
                       lse, upstream);
    AFK_LAUNCH_CHECK("afk_token_logprob_bwd");
    return AFK_OK;
}
