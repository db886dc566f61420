// Shared-prompt decode attention: ONE query row per continuation, n continuations (sampled copies or beams) per prompt row, forward only.
//
// Oracle: Qwen2Attention.forward with a cache and one new position (modeling_qwen2.py:195-234) on every one of the B0 * n rows the reference's
// _expand_inputs_for_generation makes - softmax(q k^T * scale) v over the row's prompt keys and its own generated keys.  The reference (and
// afk_attn_decode_fused on an expanded cache) reads the prompt keys of a row n times per step; here they are stored once and read once per tile of copies:
//   continuation r = b0 * n + c sees   prompt keys [prange[b0,0], prange[b0,1]) of the PROMPT cache row b0   (Kp [B0][Sp][Hkv][D], Vtp [B0][Hkv][D][spad_p])
//                                    + tail keys   [trange[r,0],  trange[r,1])  of the TAIL cache row r      (Kt [B0*n][T][Hkv][D], Vtt [B0*n][Hkv][D][spad_t])
// One partials launch, one merge launch (attention_append.hip's scheme, whose split kernel this one is copied from):
//   prompt block = (prompt row, KV head, tile of copies, key split), blockIdx.x < nsplit.  The n * G query columns (copy, head of the GQA group) are stacked
//           on the 32 columns of the MFMA tile: column c = (copy c / G of the tile, head c % G), 32 / G copies per tile (G = 7: 4 copies, 28 columns) - a
//           prompt key row fetched once serves every copy of the tile.  The interval is cut into nsplit chunks on 32-key boundaries; the four waves of a
//           block take the chunk's 32-key tiles in turn, each with its own online softmax:
//             S^T[key][c]  = K[key][:] . Q[c][:]       v_mfma_f32_32x32x16_bf16, A = 32 key rows straight from the cache, B = the 32 query columns
//             O^T[d][c]   += Vt[d][key] . P[key][c]    A = rows of the TRANSPOSED value cache, B = the bf16 probabilities in the registers the first MFMA left them in
//   tail block   = (prompt row, KV head, tile of copies, copy j of the tile), blockIdx.x = nsplit + j: the same code on the tail cache row of ONE continuation,
//           columns = its G heads (the tail is short - at most max_new_tokens keys - and every continuation has its own, so nothing can be shared)
//   either leaves one (o[D], m, l) per (continuation, head, part) in the workspace: parts 0 .. nsplit - 1 the prompt splits, part nsplit the tail.
//   THE SECOND LAUNCH folds the nsplit + 1 parts in that order with attn_decode_combine_kernel's arithmetic.  No counters, no cross-block waits, no atomics:
//   the bits depend on the inputs and nsplit only.
// A continuation that sees no key at all is a zero row (+0.0 in every element, as afk_attn_append writes it); a part that sees none leaves (-inf, 0, 0).
// What lies outside an interval is never multiplied: key rows are clamped into it (their scores are replaced by -inf with a select), value columns outside it are
// zeroed before the MFMA (0 x NaN) - cache slots behind the last key, tail slots not yet written and the pad columns of Vt may hold anything.
//
// make report (gfx950), split kernel: D = 128: 227 (G = 1) / 229 VGPRs, no AGPRs, no spill, no scratch, 66 560 B of LDS, 2 waves per SIMD - two blocks per CU
//                       (133 120 B of the 160 KiB), held there by amdgpu_waves_per_eu(2) as the append kernel is;  D = 64: 144 / 146 VGPRs, no spill, 33 792 B of
//                       LDS, 3 waves per SIMD.  Combine kernel: 20 VGPRs, no LDS, 8 waves per SIMD.
#include <limits.h>
#include "common.h"
#include "../../include/afk.h"

namespace {

constexpr float NEG_INF = -INFINITY;
constexpr float LOG2E = 1.4426950408889634f;
constexpr int SHARED_MAX_SPLITS = 64;
constexpr int SHARED_MAX_COPIES = 16;

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
// row index carried by accumulator register r in lane-half hi of a 32x32 MFMA result
#define ROW_OF(r, hi) (((r) & 3) + 8 * ((r) >> 2) + 4 * (hi))

__device__ __forceinline__ bf16x8 ld4x2(const bf16* p0, const bf16* p1) {
    const bf16x4 a = *(const bf16x4*)p0, b = *(const bf16x4*)p1;
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// workspace slot of one (continuation, head, part): o[D], m (log2 domain), l, two pad words (16-byte slots)
template <int D, int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_shared_split_kernel(
    const bf16* __restrict__ Q, int64_t q_rs, int64_t q_hs, const bf16* __restrict__ Kp, int64_t kp_bs, int64_t kp_rs, int64_t kp_hs,
    const bf16* __restrict__ Vtp, int64_t vtp_bs, int spad_p, int Sp, const bf16* __restrict__ Kt, int64_t kt_bs, int64_t kt_rs, int64_t kt_hs,
    const bf16* __restrict__ Vtt, int64_t vtt_bs, int spad_t, int T, const int* __restrict__ prange, const int* __restrict__ trange, int Hq, int Hkv,
    int n, int nsplit, float scale, float* __restrict__ ws) {
    constexpr int KS = D / 16, DT = D / 32, RT = 32 / G, SS = D + 4, DP = D / 8;
    __shared__ float part[4][D + 2][32];   // [wave][feature | m | l][column]: 66 560 B at D = 128
    const int b0 = blockIdx.z;
    const int ntile = gridDim.y / Hkv, tile = blockIdx.y % ntile, hk = blockIdx.y / ntile;   // the tiles of one (KV head, split) are neighbours in launch order
    const bool tail = (int)blockIdx.x >= nsplit;                                             // block-uniform
    const int tcopy = tile * RT + ((int)blockIdx.x - nsplit);                                // tail block: the copy it serves
    if (tail && tcopy >= n) return;                                                          // the last tile may hold fewer copies (whole block, in front of the barrier)
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int copy = tail ? tcopy : tile * RT + l31 / G, h = hk * G + l31 % G;
    const bool valid = tail ? l31 < G : (l31 < RT * G && copy < n);
    const int64_t r = (int64_t)b0 * n + min(copy, n - 1);   // the continuation (clamped: a dead column reads valid memory)
    // the block's cache row, its interval (block-uniform) and the part of the workspace slot it writes
    const int64_t rr = (int64_t)b0 * n + tcopy;   // tail blocks only
    const bf16* Kc = tail ? Kt + rr * kt_bs : Kp + b0 * kp_bs;
    const bf16* Vt = tail ? Vtt + rr * vtt_bs : Vtp + b0 * vtp_bs;
    const int64_t k_rs = tail ? kt_rs : kp_rs, k_hs = tail ? kt_hs : kp_hs;
    const int spad = tail ? spad_t : spad_p, split = tail ? 0 : (int)blockIdx.x, ns = tail ? 1 : nsplit, slot_part = tail ? nsplit : (int)blockIdx.x;
    const int* rg = tail ? trange + rr * 2 : prange + (int64_t)b0 * 2;
    int tlo = max(rg[0], 0), thi = min(rg[1], tail ? T : Sp);
    if (thi <= tlo) tlo = thi = 0;   // an empty interval: every key is dead
    const int kb = valid ? tlo : 0, ke = valid ? thi : 0;
    int c0 = 0, ntk = 0, c1 = 0;
    if (thi > tlo) {
        const int a0 = tlo & ~31;
        const int chunk = (((thi - a0) + ns - 1) / ns + 31) & ~31;
        c0 = a0 + split * chunk;
        c1 = min(c0 + chunk, thi);
        ntk = c1 > c0 ? (c1 - c0 + 31) >> 5 : 0;
    }
    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r_ = 0; r_ < 16; ++r_) oacc[dt][r_] = 0.f;
    float m = NEG_INF, l = 0.f;
    if (w < ntk) {
        const bf16* Qp = Q + r * q_rs + h * q_hs + hi * 8;
        bf16x8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(Qp + ks * 16);
        const bf16* Kb = Kc + hk * k_hs + hi * 8;
        const bf16* Vb = Vt + ((int64_t)hk * D + l31) * spad + 4 * hi;
        const float c2 = scale * LOG2E;
        bf16x8 kf[KS];
        auto load_k = [&](bf16x8(&dst)[KS], int kt) {
            const bf16* kp = Kb + (int64_t)min(max(c0 + kt * 32 + l31, tlo), thi - 1) * k_rs;   // clamped into the interval at both ends: written rows, masked below
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
            for (int r_ = 0; r_ < 16; ++r_) st[r_] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) st = MFMA(kf[ks], qf[ks], st);
            if (kt + 4 < ntk) load_k(kf, kt + 4);   // the next tile's key rows travel while this one's softmax runs
            float s[16], mx = NEG_INF;
#pragma unroll
            for (int r_ = 0; r_ < 16; ++r_) {
                const int key = key0 + ROW_OF(r_, hi);
                const bool dead = key < kb || key >= ke || key >= c1;   // c1: what lies behind belongs to the next split
                s[r_] = dead ? NEG_INF : st[r_] * c2;                    // log2 domain
                mx = fmaxf(mx, s[r_]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m, mx);
            const float m_use = (m_new == NEG_INF) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m - m_use);   // m = -inf -> 0
            float rs = 0.f;
            bf16x8 pb[2];
#pragma unroll
            for (int r_ = 0; r_ < 16; ++r_) {
                const bf16 p = (bf16)__builtin_amdgcn_exp2f(s[r_] - m_use);   // rounded to bf16 as the P.V product reads it; the row sum counts the same values
                pb[r_ >> 3][r_ & 7] = p;
                rs += (float)p;
            }
            rs += __shfl_xor(rs, 32, 64);
            l = l * alpha + rs;
            m = m_new;
            if (key0 < tlo || key0 + 32 > thi) {   // wave-uniform: a tile that sticks out of the interval - those value columns may hold anything (0 x NaN)
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
                for (int r_ = 0; r_ < 16; ++r_) oacc[dt][r_] *= alpha;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) oacc[dt] = MFMA(vf[dt][s2], pb[s2], oacc[dt]);
            }
        }
    }
    // ---- the four waves' partials meet in LDS
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r_ = 0; r_ < 16; ++r_) part[w][dt * 32 + ROW_OF(r_, hi)][l31] = oacc[dt][r_];
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
    float* slot = ws + ((r * Hq + h) * (nsplit + 1) + slot_part) * SS;   // valid: copy < n, r is the column's own continuation
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

// the second launch: thread = (entry (continuation, head), feature); the parts folded in order (prompt splits, then the tail), attn_decode_combine_kernel's arithmetic
template <int D>
__global__ __launch_bounds__(256) void attn_shared_combine_kernel(const float* __restrict__ ws, int nparts, bf16* __restrict__ O, int64_t o_rs, int64_t o_hs, int Hq,
                                                                  int64_t entries) {
    constexpr int SS = D + 4, EPB = 256 / D;
    const int64_t e = (int64_t)blockIdx.x * EPB + threadIdx.x / D;
    const int d = threadIdx.x % D;
    if (e >= entries) return;
    const int h = (int)(e % Hq);
    const int64_t r = e / Hq;
    const float* base = ws + e * nparts * SS;
    float M = NEG_INF;
    for (int s = 0; s < nparts; ++s) M = fmaxf(M, base[s * SS + D]);
    float L = 0.f, o = 0.f;
    if (M != NEG_INF) {
        for (int s = 0; s < nparts; ++s) {
            const float wgt = __builtin_amdgcn_exp2f(base[s * SS + D] - M);   // m = -inf -> 0
            L += wgt * base[s * SS + D + 1];
            o += wgt * base[s * SS + d];
        }
    }
    O[r * o_rs + h * o_hs + d] = (bf16)(L > 0.f ? o / L : 0.f);
}

}  // namespace

extern "C" int64_t afk_attn_decode_shared_workspace_floats(int B0, int n, int Hq, int D, int nsplit) { return (int64_t)B0 * n * Hq * (nsplit + 1) * (D + 4); }

extern "C" int afk_attn_decode_shared(const void* Q, int64_t q_rs, int64_t q_hs, const void* Kp, int64_t kp_bs, int64_t kp_rs, int64_t kp_hs, const void* Vtp,
                                      int64_t vtp_bs, int spad_p, int Sp, const void* Kt, int64_t kt_bs, int64_t kt_rs, int64_t kt_hs, const void* Vtt,
                                      int64_t vtt_bs, int spad_t, int T, void* O, int64_t o_rs, int64_t o_hs, const int* prange, const int* trange, int B0, int n,
                                      int Hq, int Hkv, int D, float scale, int nsplit, float* ws, int64_t ws_floats, void* stream) {
    AFK_REQUIRE(Q && O && prange && trange && ws, "afk_attn_decode_shared: null pointer");
    AFK_REQUIRE(B0 > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Sp >= 0 && T >= 0, "afk_attn_decode_shared: bad shape (B0 %d, Hq %d, Hkv %d, Sp %d, T %d)", B0, Hq, Hkv,
                Sp, T);
    AFK_REQUIRE((Sp == 0 || (Kp && Vtp)) && (T == 0 || (Kt && Vtt)), "afk_attn_decode_shared: null cache pointer (only a cache of no positions may be absent)");
    AFK_REQUIRE(D == 64 || D == 128, "afk_attn_decode_shared: head_dim %d (64 / 128 supported)", D);
    const int G = Hq / Hkv;
    AFK_REQUIRE(G == 1 || G == 2 || G == 4 || G == 7 || G == 8, "afk_attn_decode_shared: Hq / Hkv = %d (1 / 2 / 4 / 7 / 8 supported)", G);
    AFK_REQUIRE(n >= 1 && n <= SHARED_MAX_COPIES, "afk_attn_decode_shared: %d continuations per prompt row outside [1, %d]", n, SHARED_MAX_COPIES);
    AFK_REQUIRE(nsplit >= 1 && nsplit <= SHARED_MAX_SPLITS, "afk_attn_decode_shared: nsplit %d outside [1, %d]", nsplit, SHARED_MAX_SPLITS);
    AFK_REQUIRE(ws_floats >= afk_attn_decode_shared_workspace_floats(B0, n, Hq, D, nsplit),
                "afk_attn_decode_shared: workspace of %lld floats, afk_attn_decode_shared_workspace_floats says %lld", (long long)ws_floats,
                (long long)afk_attn_decode_shared_workspace_floats(B0, n, Hq, D, nsplit));
    AFK_REQUIRE(q_rs % 8 == 0 && q_hs % 8 == 0 && o_rs % 8 == 0 && o_hs % 8 == 0 && kp_bs % 8 == 0 && kp_rs % 8 == 0 && kp_hs % 8 == 0 && kt_bs % 8 == 0 &&
                    kt_rs % 8 == 0 && kt_hs % 8 == 0 && vtp_bs % 4 == 0 && vtt_bs % 4 == 0 && spad_p >= Sp && spad_t >= T && spad_p % 32 == 0 && spad_t % 32 == 0 &&
                    ((uintptr_t)ws & 15) == 0 && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)Kp & 15) == 0 && ((uintptr_t)Kt & 15) == 0 && ((uintptr_t)Vtp & 7) == 0 &&
                    ((uintptr_t)Vtt & 7) == 0,
                "afk_attn_decode_shared: strides and pointers must keep 16-byte alignment, spad_p / spad_t must be multiples of 32 that hold Sp / T");
    const int RT = 32 / G;
    const int64_t ntile = afk_cdiv(n, RT);
    AFK_REQUIRE(ntile * Hkv <= 65535 && B0 <= 65535, "afk_attn_decode_shared: %lld copy tiles x %d KV heads or %d prompt rows exceed the grid", (long long)ntile, Hkv, B0);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(nsplit + (n < RT ? n : RT)), (unsigned)(ntile * Hkv), (unsigned)B0);   // x: the prompt splits, then one tail block per copy of the tile
    const int64_t entries = (int64_t)B0 * n * Hq;
#define AFK_AS(DD, GG)                                                                                                                                          \
    hipLaunchKernelGGL((attn_shared_split_kernel<DD, GG>), grid, dim3(256), 0, st, (const bf16*)Q, q_rs, q_hs, (const bf16*)Kp, kp_bs, kp_rs, kp_hs,            \
                       (const bf16*)Vtp, vtp_bs, spad_p, Sp, (const bf16*)Kt, kt_bs, kt_rs, kt_hs, (const bf16*)Vtt, vtt_bs, spad_t, T, prange, trange, Hq, Hkv, n, \
                       nsplit, scale, ws)
#define AFK_AS_D(DD)                                                                                                                                            \
    do {                                                                                                                                                        \
        if (G == 1) AFK_AS(DD, 1);                                                                                                                              \
        else if (G == 2) AFK_AS(DD, 2);                                                                                                                         \
        else if (G == 4) AFK_AS(DD, 4);                                                                                                                         \
        else if (G == 7) AFK_AS(DD, 7);                                                                                                                         \
        else AFK_AS(DD, 8);                                                                                                                                     \
        hipLaunchKernelGGL(attn_shared_combine_kernel<DD>, dim3((unsigned)afk_cdiv(entries, 256 / DD)), dim3(256), 0, st, ws, nsplit + 1, (bf16*)O, o_rs, o_hs, \
                           Hq, entries);                                                                                                                        \
    } while (0)
    if (D == 128) AFK_AS_D(128); else AFK_AS_D(64);
#undef AFK_AS_D
#undef AFK_AS
    AFK_LAUNCH_CHECK("afk_attn_decode_shared");
    return AFK_OK;
}
