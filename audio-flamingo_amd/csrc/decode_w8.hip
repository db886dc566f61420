// FP8 decode weights (generate(decode_weights="fp8"), decode_w8.py): the one-time quantiser of a bf16 Linear weight into OCP e4m3fn codes (max finite 448, no
// infinities; never the fnuz variant) with ONE power-of-two scale per output row.  The kernels that read the copy are the W8 form of gemv_chain_kernel
// (decode_chain.hip).  The rule, restated in torch by tests/_w8_ref.py:
//     a = max |w| of the row (fp32) = m * 2^x, m in [0.5, 1);   a == 0: scale 1
//     scale = 2^e,  e = x - 9 where m <= 0.875, else x - 8      the smallest power of two with a / 2^e <= 448 (448 = 0.875 * 2^9), from the exponent and mantissa bits
//     e >= -117                                                 so that the smallest code times the scale, 2^-9 * 2^e, is a normal bf16 (rows of subnormal weights only)
//     code = RNE(w / 2^e) to e4m3fn                             the division is exact; |w / 2^e| <= 448 by construction; below 2^-10 it rounds to (signed) zero
// A power-of-two scale costs a floating format nothing, and code * scale is exactly representable in bf16: the FP8 route on weights that already lie on this grid is
// the bf16 route on the same values.  A NaN or infinite weight sets *bad (the host raises).
#include "common.h"
#include "../../include/afk.h"

namespace {

// e of a row whose largest magnitude has the fp32 bits `a_bits` (sign clear, finite)
__host__ __device__ inline int w8_row_exponent(uint32_t a_bits) {
    if (a_bits == 0) return 0;
    int E = (int)(a_bits >> 23);
    uint32_t man = a_bits & 0x7fffffu;
    if (E == 0) {   // an fp32 subnormal (so is every bf16 subnormal): shift the leading one into the hidden-bit place
        int sh = 0;
        while (!(man & 0x800000u)) { man <<= 1; ++sh; }
        man &= 0x7fffffu;
        E = 1 - sh;
    }
    const int x = E - 126;                             // a = 1.f * 2^(E - 127) = (1.f / 2) * 2^x
    const int e = man <= 0x600000u ? x - 9 : x - 8;    // 1.f <= 1.75  <=>  m <= 0.875
    return e < -117 ? -117 : e;
}

// round-to-nearest-even of a finite fp32 with |v| <= 448 to e4m3fn (bias 7, subnormals in units of 2^-9), in integer arithmetic
__host__ __device__ inline uint32_t w8_encode(uint32_t v_bits) {
    const uint32_t sign = (v_bits >> 24) & 0x80u, a = v_bits & 0x7fffffffu;
    const int E = (int)(a >> 23);
    uint32_t code;
    if (E >= 121) {   // >= 2^-6: normal in e4m3; drop 20 mantissa bits, ties to even, a carry walks into the exponent
        code = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
        if (code > 0x7eu) code = 0x7eu;   // saturate at 448 (never reached: |v| <= 448)
    } else if (E < 117) {   // below 2^-10, half the smallest subnormal
        code = 0;
    } else {   // units of 2^-9: sig * 2^(E - 150) / 2^-9 = the 24-bit significand shifted right by 141 - E places (21 .. 24), ties to even; 8 = the smallest normal
        const uint32_t sig = (a & 0x7fffffu) | 0x800000u;
        const int sh = 141 - E;
        const uint32_t q = sig >> sh, rem = sig & ((1u << sh) - 1u), halfway = 1u << (sh - 1);
        code = q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u);
    }
    return sign | code;
}

// one block per row: the row's largest magnitude (bf16 magnitudes order like their bit patterns), then the codes, a byte per thread and store (one-time work: no vector loads)
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const bf16* __restrict__ W, int64_t ldw, int K, uint8_t* __restrict__ Q, int64_t ldq, float* __restrict__ scale,
                                                                int* __restrict__ bad) {
    __shared__ uint32_t smax[4];
    const int row = blockIdx.x, t = threadIdx.x;
    const unsigned short* w = (const unsigned short*)(W + (int64_t)row * ldw);
    uint32_t mx = 0;
    for (int k = t; k < K; k += 256) {
        const uint32_t b = w[k] & 0x7fffu;
        mx = b > mx ? b : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((t & 63) == 0) smax[t >> 6] = mx;
    __syncthreads();
    mx = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    if (mx >= 0x7f80u) {   // NaN or infinity in the row: nothing sensible to store
        if (t == 0) { *bad = 1; scale[row] = 1.f; }
        mx = 0;
    }
    const int e = w8_row_exponent(mx << 16);
    if (t == 0 && mx < 0x7f80u) scale[row] = ldexpf(1.f, e);
    uint8_t* q = Q + (int64_t)row * ldq;
    for (int k = t; k < K; k += 256) {
        const uint32_t b = w[k];
        const bool finite = (b & 0x7f80u) != 0x7f80u;
        const float v = ldexpf(__uint_as_float((finite ? b : 0u) << 16), -e);   // exact (a power of two) down to the fp32 subnormals, far below where the codes end
        q[k] = (uint8_t)w8_encode(__float_as_uint(v));
    }
}

}  // namespace

#ifndef AFK_W8_HOST_TEST
extern "C" int afk_quantize_rows_fp8(const void* W, int64_t ldw, int N, int K, void* Q, int64_t ldq, float* scale, int* bad, void* stream) {
    AFK_REQUIRE(W && Q && scale && bad && N > 0 && K > 0 && ldw >= K && ldq >= K, "afk_quantize_rows_fp8: bad arguments (ldw >= K, ldq >= K)");
    hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const bf16*)W, ldw, K, (uint8_t*)Q, ldq, scale, bad);
    AFK_LAUNCH_CHECK("afk_quantize_rows_fp8");
    return AFK_OK;
}
#endif
