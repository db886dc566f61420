// Append attention: a tile of NEW query rows per sample against a long KV cache, split-KV, forward only.
//
// Oracle: Qwen2Attention.forward with a cache and more than one new position (modeling_qwen2.py:195-234): softmax(q k^T * scale) v, every new row over the
// cached positions and the new rows up to itself.  This is the shape of a chat turn: n ~ 8 .. 1 000 rows behind thousands of cached keys.  The interval kernel
// (attention.hip, afk_xattn_fwd) gives it one wave per 32 query rows of ONE head that walks all keys serially - 56 waves at the AF3 geometry for a 64-row turn.
// Here attn_decode_gmma_kernel's idea (attention_decode.hip) is taken from one query row to a tile of them:
//   block = (sample, KV head, query-row tile, key split).  The G = Hq / Hkv query heads of the group are stacked on the 32 columns of the MFMA tile:
//           column c = (row c / G of the tile, head c % G), 32 / G rows per tile (G = 7: 4 rows, 28 columns) - a key row fetched once serves all of them.
//   split   the hull [tlo, thi) of the tile's key intervals (NOT the whole cache: a causal tile stops at its own last row) is cut into nsplit chunks on
//           32-key boundaries; the four waves of a block take the 32-key tiles of the chunk in turn, each with its own online softmax:
//             S^T[key][c]  = K[key][:] . Q[c][:]       v_mfma_f32_32x32x16_bf16, A = 32 key rows straight from the cache, B = the 32 query columns
//             O^T[d][c]   += Vt[d][key] . P[key][c]    A = rows of the TRANSPOSED value cache, B = the bf16 probabilities in the registers the first MFMA
//                                                      left them in (the k index of an MFMA may be permuted as long as both operands agree)
//   merge   the four waves' (m, l, o[D]) meet in LDS in wave order; the block leaves one (o[D], m, l) per (row, head, split) in the workspace.
//   A SECOND LAUNCH folds the splits in split order with attn_decode_combine_kernel's arithmetic.  No counters, no cross-block waits, no atomics: the bits
//   depend on the inputs and nsplit only.
// Visibility is afk_xattn_fwd's interval contract: row i of sample b sees keys [krange[b,i,0], krange[b,i,1]), read on the device (capturable); an empty
// interval is a zero row (+0.0 in every element, as afk_xattn_fwd writes it).  A split whose chunk misses a row leaves (-inf, 0, 0) for it.
// What lies outside the hull is never multiplied: key rows are clamped into it (their scores are replaced by -inf with a select), value columns outside
// it are zeroed before the MFMA (0 x NaN) - cache slots behind the last key and the pad columns of Vt may hold anything.
#include <limits.h>
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr float NEG_INF = -INFINITY;
constexpr float LOG2E = 1.4426950408889634f;
constexpr int APPEND_MAX_SPLITS = 64;

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
// row index carried by accumulator register r in lane-half hi of a 32x32 MFMA result
#define ROW_OF(r, hi) (((r) & 3) + 8 * ((r) >> 2) + 4 * (hi))

__device__ __forceinline__ bf16x8 ld4x2(const bf16* p0, const bf16* p1) {
    const bf16x4 a = *(const bf16x4*)p0, b = *(const bf16x4*)p1;
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// workspace slot of one (sample, head, row, split): o[D], m (log2 domain), l, two pad words (16-byte slots)
// amdgpu_waves_per_eu(2): left alone the D = 128 form takes 218 VGPRs + 80 AGPRs = one block per CU; held to two waves per SIMD it fits 229 VGPRs without a
// spill, and two blocks (2 x 66 560 B of LDS) share a CU - a wave's key / value round trips then overlap the other block's MFMAs
template <int D, int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_append_split_kernel(const bf16* __restrict__ Q, int64_t q_bs, int64_t q_hs, int64_t q_rs,
                                                                const bf16* __restrict__ Kc, int64_t k_bs, int64_t k_rs, int64_t k_hs,
                                                                const bf16* __restrict__ Vt, int64_t vt_bs, int spad, const int* __restrict__ krange,
                                                                int Hq, int Hkv, int n, float scale, float* __restrict__ ws) {
    constexpr int KS = D / 16, DT = D / 32, RT = 32 / G, SS = D + 4, DP = D / 8;
    __shared__ float part[4][D + 2][32];   // [wave][feature | m | l][column]: 66 560 B at D = 128
    const int split = blockIdx.x, nsplit = gridDim.x, b = blockIdx.z;
    const int ntile = gridDim.y / Hkv, tile = blockIdx.y % ntile, hk = blockIdx.y / ntile;   // the tiles of one (KV head, split) are neighbours in launch order
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int row = tile * RT + l31 / G, h = hk * G + l31 % G;
    const bool valid = l31 < RT * G && row < n;
    const int rowc = min(row, n - 1);
    int kb = 0, ke = 0;
    if (valid) {
        kb = max(krange[((int64_t)b * n + rowc) * 2], 0);
        ke = min(krange[((int64_t)b * n + rowc) * 2 + 1], spad);
    }
    if (ke <= kb) kb = ke = 0;   // an empty interval: every key is dead
    // hull of the tile's intervals (the same in every lane of every wave: block-uniform)
    int tlo = ke > kb ? kb : INT_MAX, thi = ke;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        tlo = min(tlo, __shfl_xor(tlo, o, 64));
        thi = max(thi, __shfl_xor(thi, o, 64));
    }
    tlo = __builtin_amdgcn_readfirstlane(tlo);
    thi = __builtin_amdgcn_readfirstlane(thi);
    int c0 = 0, ntk = 0, c1 = 0;
    if (thi > tlo) {
        const int a0 = tlo & ~31;
        const int chunk = (((thi - a0) + nsplit - 1) / nsplit + 31) & ~31;
        c0 = a0 + split * chunk;
        c1 = min(c0 + chunk, thi);
        ntk = c1 > c0 ? (c1 - c0 + 31) >> 5 : 0;
    }
    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    float m = NEG_INF, l = 0.f;
    if (w < ntk) {
        const bf16* Qp = Q + b * q_bs + h * q_hs + (int64_t)rowc * q_rs + hi * 8;
        bf16x8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(Qp + ks * 16);
        const bf16* Kb = Kc + b * k_bs + hk * k_hs + hi * 8;
        const bf16* Vb = Vt + b * vt_bs + ((int64_t)hk * D + l31) * spad + 4 * hi;
        const float c2 = scale * LOG2E;
        bf16x8 kf[KS];
        auto load_k = [&](bf16x8(&dst)[KS], int kt) {
            const bf16* kp = Kb + (int64_t)min(c0 + kt * 32 + l31, thi - 1) * k_rs;   // clamped into the hull: valid memory, masked below
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dst[ks] = *(const bf16x8*)(kp + ks * 16);
        };
        load_k(kf, w);
        for (int kt = w; kt < ntk; kt += 4) {
            const int key0 = c0 + kt * 32;   // % 32 == 0, < thi <= spad: the tile's 32 value columns lie inside the pitch
            bf16x8 vf[DT][2];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bf16* vp = Vb + (int64_t)dt * 32 * spad + key0;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) vf[dt][s2] = ld4x2(vp + 16 * s2, vp + 16 * s2 + 8);
            }
            f32x16 st;
#pragma unroll
            for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) st = MFMA(kf[ks], qf[ks], st);
            if (kt + 4 < ntk) load_k(kf, kt + 4);   // the next tile's key rows travel while this one's softmax runs
            float s[16], mx = NEG_INF;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + ROW_OF(r, hi);
                const bool dead = key < kb || key >= ke || key >= c1;   // c1: what lies behind belongs to the next split
                s[r] = dead ? NEG_INF : st[r] * c2;                      // log2 domain
                mx = fmaxf(mx, s[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m, mx);
            const float m_use = (m_new == NEG_INF) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m - m_use);   // m = -inf -> 0
            float rs = 0.f;
            bf16x8 pb[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bf16 p = (bf16)__builtin_amdgcn_exp2f(s[r] - m_use);   // rounded to bf16 as the P.V product reads it; the row sum counts the same values
                pb[r >> 3][r & 7] = p;
                rs += (float)p;
            }
            rs += __shfl_xor(rs, 32, 64);
            l = l * alpha + rs;
            m = m_new;
            if (key0 < tlo || key0 + 32 > thi) {   // wave-uniform: a tile that sticks out of the hull - those value columns may hold anything (0 x NaN)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int key = key0 + 16 * s2 + 8 * (e >> 2) + 4 * hi + (e & 3);
                            if (key < tlo || key >= thi) vf[dt][s2][e] = (bf16)0.f;
                        }
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) oacc[dt] = MFMA(vf[dt][s2], pb[s2], oacc[dt]);
            }
        }
    }
    // ---- the four waves' partials meet in LDS
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[w][dt * 32 + ROW_OF(r, hi)][l31] = oacc[dt][r];
    if (hi == 0) {
        part[w][D][l31] = m;
        part[w][D + 1][l31] = l;
    }
    __syncthreads();
    if (!valid) return;
    // thread = (column l31, feature eighth 2 w + hi); folded in wave order
    const int p8 = 2 * w + hi;
    float M = NEG_INF;
#pragma unroll
    for (int u = 0; u < 4; ++u) M = fmaxf(M, part[u][D][l31]);
    float wg[4], L = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        wg[u] = (M == NEG_INF) ? 0.f : __builtin_amdgcn_exp2f(part[u][D][l31] - M);   // m = -inf -> 0
        L += wg[u] * part[u][D + 1][l31];
    }
    float* slot = ws + ((((int64_t)b * Hq + h) * n + row) * nsplit + split) * SS;
#pragma unroll
    for (int q4 = 0; q4 < DP / 4; ++q4) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = p8 * DP + q4 * 4 + e;
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) a += wg[u] * part[u][d][l31];
            o[e] = a;
        }
        *(f32x4*)(slot + p8 * DP + q4 * 4) = o;
    }
    if (p8 == 0) {
        slot[D] = M;
        slot[D + 1] = L;
    }
}

// the second launch: thread = (entry (sample, head, row), feature); the splits folded in split order, attn_decode_combine_kernel's arithmetic
template <int D>
__global__ __launch_bounds__(256) void attn_append_combine_kernel(const float* __restrict__ ws, int nsplit, bf16* __restrict__ O, int64_t o_bs, int64_t o_hs,
                                                                  int64_t o_rs, int Hq, int n, int64_t entries) {
    constexpr int SS = D + 4, EPB = 256 / D;
    const int64_t e = (int64_t)blockIdx.x * EPB + threadIdx.x / D;
    const int d = threadIdx.x % D;
    if (e >= entries) return;
    const int i = (int)(e % n), h = (int)((e / n) % Hq), b = (int)(e / n / Hq);
    const float* base = ws + e * nsplit * SS;
    float M = NEG_INF;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, base[s * SS + D]);
    float L = 0.f, o = 0.f;
    if (M != NEG_INF) {
        for (int s = 0; s < nsplit; ++s) {
            const float wgt = __builtin_amdgcn_exp2f(base[s * SS + D] - M);   // m = -inf -> 0
            L += wgt * base[s * SS + D + 1];
            o += wgt * base[s * SS + d];
        }
    }
    O[b * o_bs + h * o_hs + (int64_t)i * o_rs + d] = (bf16)(L > 0.f ? o / L : 0.f);
}

}  // namespace

extern "C" int64_t afk_attn_append_workspace_floats(int B, int Hq, int n, int D, int nsplit) { return (int64_t)B * Hq * n * nsplit * (D + 4); }

extern "C" int afk_attn_append(const void* Q, int64_t q_bs, int64_t q_hs, int64_t q_rs, const void* Kc, int64_t k_bs, int64_t k_rs, int64_t k_hs,
                               const void* Vt, int64_t vt_bs, int spad, void* O, int64_t o_bs, int64_t o_hs, int64_t o_rs, const int* krange, int B,
                               int Hq, int Hkv, int n, int D, float scale, int nsplit, float* ws, int64_t ws_floats, void* stream) {
    AFK_REQUIRE(Q && Kc && Vt && O && krange && ws, "afk_attn_append: null pointer");
    AFK_REQUIRE(B > 0 && Hq > 0 && Hkv > 0 && n > 0 && Hq % Hkv == 0, "afk_attn_append: bad shape (B %d, Hq %d, Hkv %d, n %d)", B, Hq, Hkv, n);
    AFK_REQUIRE(D == 64 || D == 128, "afk_attn_append: head_dim %d (64 / 128 supported)", D);
    const int G = Hq / Hkv;
    AFK_REQUIRE(G == 1 || G == 2 || G == 4 || G == 7 || G == 8, "afk_attn_append: Hq / Hkv = %d (1 / 2 / 4 / 7 / 8 supported)", G);
    AFK_REQUIRE(nsplit >= 1 && nsplit <= APPEND_MAX_SPLITS, "afk_attn_append: nsplit %d outside [1, %d]", nsplit, APPEND_MAX_SPLITS);
    AFK_REQUIRE(ws_floats >= afk_attn_append_workspace_floats(B, Hq, n, D, nsplit), "afk_attn_append: workspace of %lld floats, afk_attn_append_workspace_floats says %lld",
                (long long)ws_floats, (long long)afk_attn_append_workspace_floats(B, Hq, n, D, nsplit));
    AFK_REQUIRE(q_bs % 8 == 0 && q_hs % 8 == 0 && q_rs % 8 == 0 && k_bs % 8 == 0 && k_rs % 8 == 0 && k_hs % 8 == 0 && vt_bs % 4 == 0 && spad > 0 && spad % 32 == 0 &&
                    ((uintptr_t)ws & 15) == 0,
                "afk_attn_append: strides must keep 16-byte alignment, spad must be a multiple of 32");
    const int64_t ntile = afk_cdiv(n, 32 / G);
    AFK_REQUIRE(ntile * Hkv <= 65535 && B <= 65535, "afk_attn_append: %lld query tiles x %d KV heads exceed the grid", (long long)ntile, Hkv);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nsplit, (unsigned)(ntile * Hkv), (unsigned)B);
    const int64_t entries = (int64_t)B * Hq * n;
#define AFK_AA(DD, GG)                                                                                                                                     \
    hipLaunchKernelGGL((attn_append_split_kernel<DD, GG>), grid, dim3(256), 0, st, (const bf16*)Q, q_bs, q_hs, q_rs, (const bf16*)Kc, k_bs, k_rs, k_hs,    \
                       (const bf16*)Vt, vt_bs, spad, krange, Hq, Hkv, n, scale, ws)
#define AFK_AA_D(DD)                                                                                                                                       \
    do {                                                                                                                                                   \
        if (G == 1) AFK_AA(DD, 1);                                                                                                                         \
        else if (G == 2) AFK_AA(DD, 2);                                                                                                                    \
        else if (G == 4) AFK_AA(DD, 4);                                                                                                                    \
        else if (G == 7) AFK_AA(DD, 7);                                                                                                                    \
        else AFK_AA(DD, 8);                                                                                                                                \
        hipLaunchKernelGGL(attn_append_combine_kernel<DD>, dim3((unsigned)afk_cdiv(entries, 256 / DD)), dim3(256), 0, st, ws, nsplit, (bf16*)O, o_bs, o_hs, \
                           o_rs, Hq, n, entries);                                                                                                          \
    } while (0)
    if (D == 128) AFK_AA_D(128); else AFK_AA_D(64);
#undef AFK_AA_D
#undef AFK_AA
    AFK_LAUNCH_CHECK("afk_attn_append");
    return AFK_OK;
}
