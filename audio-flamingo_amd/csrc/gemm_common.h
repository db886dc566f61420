// Shared pieces of the NT GEMM kernels (argument block, tile->workgroup mapping, fused epilogue).
#pragma once
#include "common.h"
#include "../../include/afk.h"

struct GemmArgs {
    const bf16* A;
    const bf16* B;
    void* C;
    void* C2;  // optional second output: pre-activation (bf16) when AFK_GEMM_GELU is set
    const bf16* bias;
    const bf16* R;
    int64_t lda, ldb, ldc, ldr;
    int M, N, K;
    int ntm, ntn;
    int flags;
    int res_mod;  // residual row = m % res_mod when > 0 (broadcast table, e.g. embed_positions)
    float alpha;
    int gm;  // M-tiles per rasterization group (L2 locality)
    int splits;  // split-K: blockIdx.y = split, raw fp32 partial sums go to ws[split][M][N]
    float* ws;
    int wide;    // 16-byte epilogue accesses are legal (N % 8 == 0 and every epilogue pointer / leading dimension 16-byte aligned)
    // AFK_GEMM_ROPE (afk_gemm_nt_bf16_rope): rotate-half RoPE on output columns [0, rope_cols), heads of 128 columns
    const bf16* rope_cos;
    const bf16* rope_sin;
    const int* rope_pos;   // [M] or null (row % rope_S)
    int rope_S, rope_cols;
    const bf16* rope_cos_lanes;   // afk_rope_lanes_table(form 1) copies (nullable): element ((rb * 16 + c) * 32 + l31) * 8 + e = table[32 rb + l31][8 c + e]
    const bf16* rope_sin_lanes;
};

// Probe bits of GemmArgs::gm (bit 6 = kernel WITHOUT its epilogue: wrong results; bit 7 = raw dispatch order; bit 8, read by the launchers only = the
// OLDLOOP instantiation of the 256x256 kernels, i.e. their previous K loop: afk_gemm_set_variant(15), profiles/gemm_tail.md) and the three rejected 256x256
// schedules (gemm256w4 / gemm256f8 / gemm256p.hip, profiles/r02_gemm_probes.md) exist only in -DAFK_PROBES builds (make PROBES=1).  The
// default library compiles the branches away and afk_gemm_set_variant() rejects the values that select them.
#ifdef AFK_PROBES
#define AFK_GM_NOEPI(p) (((p).gm & 0x40) != 0)
#define AFK_GM_RAW(p) (((p).gm & 0x80) != 0)
#define AFK_GM_OLDLOOP(p) (((p).gm & 0x100) != 0)
#else
#define AFK_GM_NOEPI(p) false
#define AFK_GM_RAW(p) false
#endif

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

// workgroup -> tile: XCD-contiguous (bijective remap of the round-robin dispatch) then grouped along M so that
// the tiles resident on one XCD share A and B panels through that XCD's private L2.
__device__ __forceinline__ void gemm_tile_of(const GemmArgs& p, int bid, int nwg, int& tm, int& tn) {
    const int xcd = bid & 7, idx = bid >> 3, q = nwg >> 3, r = nwg & 7;
    const int swz = AFK_GM_RAW(p) ? bid : (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;  // bit 7 of gm (probe builds): raw dispatch order
    const int GM = (p.gm & 0x3f) > 0 ? (p.gm & 0x3f) : 4;
    const int per_group = GM * p.ntn;
    const int g = swz / per_group, rem = swz - g * per_group;
    const int first_m = g * GM;
    const int gsz = min(p.ntm - first_m, GM);
    tm = first_m + rem % gsz;
    tn = rem / gsz;
}
__device__ __forceinline__ void gemm_tile_of_block(const GemmArgs& p, int& tm, int& tn) { gemm_tile_of(p, blockIdx.x, gridDim.x, tm, tn); }

// epilogue for W (4 or 8) consecutive n of one row m (values already hold the fp32 accumulators)
// order: *alpha, +bias[n] -> (round bf16, write preact, GELU-erf) -> (round bf16, +residual) -> (+C if ACCUM) -> store
// F >= 0: the epilogue flags are a compile-time constant (one kernel instantiation per epilogue the training step uses) - the kernel then
// carries ONLY that epilogue.  With the runtime form (F = -1) every one of the 16 store sites of a wave inlines all variants (erf GELU,
// SwiGLU backward with its divides, fp32 / accumulate forms): ~30 000 instructions, ~200 KB of code behind a 350-instruction K loop, and the
// plain path hops through it once per tile - the instruction cache (64 KB per two CUs) misses all the way (profiles/r02_gemm_probes.md §10).
template <int W, int F = -1>
__device__ __forceinline__ void gemm_epilogue_store(const GemmArgs& p, int m, int n, float* v) {
    typedef __attribute__((ext_vector_type(W))) __bf16 bvec;
    typedef __attribute__((ext_vector_type(W))) float fvec;
    const int flags = F >= 0 ? F : p.flags;
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] *= p.alpha;
    if (flags & AFK_GEMM_BIAS) {
        const bvec bv = *(const bvec*)(p.bias + n);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] += (float)bv[e];
    }
    if (flags & AFK_GEMM_GELU) {
        // oracle applies GELU to the bf16-rounded Linear output
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = rbf(v[e]);
        if (p.C2) {
            bvec pre;
#pragma unroll
            for (int e = 0; e < W; ++e) pre[e] = (bf16)v[e];
            *(bvec*)((bf16*)p.C2 + (int64_t)m * p.ldc + n) = pre;
        }
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = gelu_f(v[e]);
    }
    if (flags & AFK_GEMM_SWIGLU_BWD) {
        // v = d(silu(gate)*up) for columns n.. of the SwiGLU output (this GEMM is the down-projection dgrad).  R = the saved
        // [rows, 2N] gate|up pre-activations; the two gradients go to C[m, n] (gate) and C[m, N + n] (up): the [rows, N] intermediate
        // never exists in HBM.  Same arithmetic as silu_mul_bwd_kernel on the bf16-rounded GEMM result (bit-identical to the
        // two-kernel form).
        const bvec gv = *(const bvec*)(p.R + (int64_t)m * p.ldr + n);
        const bvec uv = *(const bvec*)(p.R + (int64_t)m * p.ldr + p.N + n);
        bvec og, ou;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const float gf = (float)gv[e], uf = (float)uv[e], df = rbf(v[e]);
            const float s = sigmoid_f(gf);
            og[e] = (bf16)(df * uf * (s * (1.f + gf * (1.f - s))));
            ou[e] = (bf16)(df * (gf * s));
        }
        bf16* cp = (bf16*)p.C + (int64_t)m * p.ldc + n;
        *(bvec*)cp = og;
        *(bvec*)(cp + p.N) = ou;
        return;
    }
    if (flags & AFK_GEMM_RESIDUAL) {
        const int rm = p.res_mod > 0 ? m % p.res_mod : m;
        const bvec rv = *(const bvec*)(p.R + (int64_t)rm * p.ldr + n);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = rbf(v[e]) + (float)rv[e];
    }
    if (flags & AFK_GEMM_OUT_F32) {
        float* cp = (float*)p.C + (int64_t)m * p.ldc + n;
        fvec o;
        if (flags & AFK_GEMM_ACCUM) {
            o = *(const fvec*)cp;
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] += v[e];
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] = v[e];
        }
        *(fvec*)cp = o;
    } else {
        bf16* cp = (bf16*)p.C + (int64_t)m * p.ldc + n;
        if (flags & AFK_GEMM_ACCUM) {
            const bvec old = *(const bvec*)cp;
#pragma unroll
            for (int e = 0; e < W; ++e) v[e] += (float)old[e];
        }
        bvec o;
#pragma unroll
        for (int e = 0; e < W; ++e) o[e] = (bf16)v[e];
        *(bvec*)cp = o;
    }
}
__device__ __forceinline__ void gemm_epilogue_store4(const GemmArgs& p, int m, int n, float v[4]) { gemm_epilogue_store<4, -1>(p, m, n, v); }

// ---------------------------------------------------------------- MFMA shape of the 256x256 kernels (MF = 32: v_mfma_f32_32x32x16_bf16, MF = 16: v_mfma_f32_16x16x32_bf16)
// Only the fragment a lane reads, the MFMA calls and the accumulator indexing depend on MF; LDS images, LDS-DMA lists, the vmcnt ladder, the barriers and
// the wave -> 128 x 64 block map do not.  The lane maps below are mirrored line by line in tests/test_gemm_frag_map_cpu.py (bank conflicts, bijection).
//
// k-contiguous image (128-byte rows, chunk c of row r at c ^ ((r >> 1) & 7)), one ds_read_b128 per fragment:
//   MF = 32: fragment (32-row tile, k-step s of 16):  row = 32 tile + (lane & 31),  chunk = 2 s + (lane >> 5),  s = 0..3
//   MF = 16: fragment (16-row tile, k-step s of 32):  row = 16 tile + (lane & 15),  chunk = 4 s + (lane >> 4),  s = 0..1
// In both (row >> 1) & 7 == (lane >> 1) & 7, so the swizzle term stays a lane constant.  Fragment x = 0..3 of a 32-row tile is k-step x (MF = 32) or
// 16-row half x >> 1, k-step x & 1 (MF = 16): eight fragments per 64 rows x 64 k either way.
template <int MF>
__device__ __forceinline__ int gemm_frag_row(int lane) { return MF == 16 ? (lane & 15) : (lane & 31); }   // + 32 * tile (+ 16 * (x >> 1) for MF = 16)
template <int MF>
__device__ __forceinline__ int gemm_frag_koff(int x, int lane) {   // byte offset inside the 128-byte row
    const int chunk = MF == 16 ? 4 * (x & 1) + (lane >> 4) : 2 * x + (lane >> 5);
    return (chunk ^ ((lane >> 1) & 7)) << 4;
}
template <int MF>
__device__ __forceinline__ constexpr int gemm_frag_rowoff(int x) { return MF == 16 ? (x >> 1) * 16 : 0; }   // rows added to the 32-row tile base by fragment x

// Accumulators of a wave's 128 (m) x 64 (n) block: 128 VGPRs in both shapes.  mfma(bfrag, afrag, acc) leaves in a lane
//   MF = 32: block (i, j) of 32 x 32: row 32 i + (lane & 31), registers 4 q + {0..3} = columns 32 j + 8 q + 4 (lane >> 5) + {0..3}
//   MF = 16: tile (it, jt) of 16 x 16: row 16 it + (lane & 15), registers {0..3}     = columns 16 jt + 4 (lane >> 4) + {0..3}
// block(i, j) hands one 32 x 32 block to the epilogue as 16 registers b[8 t + 4 h + e]:
//   MF = 32: the accumulator itself (t = q >> 1, h = q & 1)
//   MF = 16: tile (2 i + h, 2 j + t), so that the wide form below is the same code with v_permlane16_swap in place of v_permlane32_swap
// Keeps the computation of a lane value where the source puts it: without a use in front of the first barrier the compiler sinks the prologue's set-up
// (fragment offsets, accumulator zeroing) behind that barrier, out of the shadow of the first LDS-DMA loads and onto the critical path of the first tile.
template <class T>
__device__ __forceinline__ void afk_pin(T& v) { asm volatile("" : "+v"(v)); }

template <int MF>
struct GemmAcc;
template <>
struct GemmAcc<32> {
    f32x16 v[4][2];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) v[i][j][e] = 0.f;
    }
    __device__ __forceinline__ void pin() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) afk_pin(v[i][j]);
    }
    // acc[i][j] += A rows (32 i ..) x B rows (32 j ..) over the k of fragment pair (xa, xb): one MFMA, xa == xb == k-step
    __device__ __forceinline__ void mma(int i, int j, const bf16x8& b, const bf16x8& a) { v[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, v[i][j], 0, 0, 0); }
    __device__ __forceinline__ f32x16 block(int i, int j) const { return v[i][j]; }
};
template <>
struct GemmAcc<16> {
    f32x4 v[8][4];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[i][j][e] = 0.f;
    }
    __device__ __forceinline__ void pin() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) afk_pin(v[i][j]);
    }
    __device__ __forceinline__ void mma(int it, int jt, const bf16x8& b, const bf16x8& a) { v[it][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, v[it][jt], 0, 0, 0); }
    __device__ __forceinline__ f32x16 block(int i, int j) const {
        f32x16 b;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e) b[8 * t + 4 * h + e] = v[2 * i + h][2 * j + t][e];
        return b;
    }
};

// One lane-pair exchange of the wide epilogue: registers x = b[8 t + e] and y = b[8 t + 4 + e] of a block go in, and every lane comes out with
// lo = column c + e and hi = column c + 4 + e of ONE row, c = nb + 16 t + 8 (lane >> 5), row = mb + (lane & 31) - in both shapes:
//   MF = 32: v_permlane32_swap trades lanes l and l + 32 (same row, columns 4 apart);
//   MF = 16: v_permlane16_swap trades lanes l and l + 16 for (lane >> 4) even: x, y are the SAME columns 16 t + 4 g + e of the row tiles h = 0 and
//            h = 1; after the swap even-g lanes hold row tile 0 at columns 4 g + e and 4 (g + 1) + e, odd-g lanes row tile 1 at 4 (g - 1) + e and
//            4 g + e: row 16 (g & 1) + (lane & 15) = lane & 31, first column 8 (g >> 1) = 8 (lane >> 5).
template <int MF>
__device__ __forceinline__ void gemm_lane_swap(float x, float y, float& lo, float& hi) {
    if constexpr (MF == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
        lo = __uint_as_float(r[0]);
        hi = __uint_as_float(r[1]);
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
        lo = __uint_as_float(r[0]);      // lo lanes: own q=2t ; hi lanes: partner's q=2t+1
        hi = __uint_as_float(r[1]);      // lo lanes: partner's q=2t ; hi lanes: own q=2t+1
    }
}
// (row, column) of the 4 consecutive values b[8 t + 4 h + 0..3] a lane holds BEFORE the exchange (narrow stores, split-K partials)
template <int MF>
__device__ __forceinline__ void gemm_quad_pos(int lane, int t, int h, int& row, int& col) {
    if (MF == 16) {
        row = 16 * h + (lane & 15);
        col = 16 * t + 4 * (lane >> 4);
    } else {
        row = lane & 31;
        col = 8 * (2 * t + h) + 4 * (lane >> 5);
    }
}

// One 32 (m) x 32 (n) result block of a wave (rows mb.., columns nb..; b as GemmAcc::block lays it out).  Wide form (p.wide: every pointer / leading
// dimension of the epilogue keeps 16-byte alignment): lane pairs trade registers (gemm_lane_swap) so that each lane owns 8 CONSECUTIVE columns
// (nb + 16t + 8 (lane >> 5) + 0..7) of row mb + (lane & 31) - 16-byte stores and 16-byte bias / residual loads, half as many memory instructions as the
// 8-byte form.  Split-K partials keep the 4-wide form.  Every lane takes part in the exchange, so rows past M are masked at the store, not by an early exit.
// F >= 0 (specialised instantiation): the launcher guarantees p.wide and p.splits <= 1.  F = -2: split-K partial sums only.
template <int F, int MF>
__device__ __forceinline__ void gemm_store_block32_body(const GemmArgs& p, int mb, int nb, int lane, const f32x16& b);
// The runtime-flag form (F = -1: narrow stores, fp32 output, epilogues outside the training step) as ONE out-of-line function per kernel
// image: inlined at the 8 store sites of a 256x256 wave it made the generic instantiations of the 2-waves-per-SIMD kernels spill 730 VGPRs
// to scratch; the accumulator block travels by value in 16 VGPRs.
template <int MF>
static __device__ __noinline__ void gemm_store_block32_generic(const GemmArgs& p, int mb, int nb, int lane, f32x16 b) {
    gemm_store_block32_body<-1, MF>(p, mb, nb, lane, b);
}
template <int F = -1, int MF = 32>
__device__ __forceinline__ void gemm_store_block32(const GemmArgs& p, int mb, int nb, int lane, const f32x16& b) {
    if constexpr (F == -1) gemm_store_block32_generic<MF>(p, mb, nb, lane, b);
    else gemm_store_block32_body<F, MF>(p, mb, nb, lane, b);
}
template <int F, int MF>
__device__ __forceinline__ void gemm_store_block32_body(const GemmArgs& p, int mb, int nb, int lane, const f32x16& b) {
    if (F == -2 || (F == -1 && p.splits > 1)) {  // F = -2: split-K launch, fp32 partial sums only
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int row, col;
                gemm_quad_pos<MF>(lane, t, h, row, col);
                const int m = mb + row, n = nb + col;
                if (m >= p.M || n >= p.N) continue;
                const f32x4 o = {b[8 * t + 4 * h], b[8 * t + 4 * h + 1], b[8 * t + 4 * h + 2], b[8 * t + 4 * h + 3]};
                *(f32x4*)(p.ws + ((int64_t)blockIdx.y * p.M + m) * p.N + n) = o;
            }
        return;
    }
    if constexpr (F == -2) return;
    if (F >= 0 || p.wide) {
        const int m = mb + (lane & 31);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) gemm_lane_swap<MF>(b[8 * t + e], b[8 * t + 4 + e], v[e], v[4 + e]);
            const int n = nb + 16 * t + 8 * (lane >> 5);
            if (m < p.M && n < p.N) gemm_epilogue_store<8, F>(p, m, n, v);
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int row, col;
            gemm_quad_pos<MF>(lane, t, h, row, col);
            const int m = mb + row, n = nb + col;
            if (m >= p.M || n >= p.N) continue;
            float v[4] = {b[8 * t + 4 * h], b[8 * t + 4 * h + 1], b[8 * t + 4 * h + 2], b[8 * t + 4 * h + 3]};
            gemm_epilogue_store<4, F>(p, m, n, v);
        }
}

// Which MFMA shapes of each 256x256 kernel the library carries: bit 0 = 32x32x16, bit 1 = 16x16x32.  The shape that the per-shape table of
// profiles/gemm_mfma_shape_ab.md does not justify is compiled under make PROBES=1 only, and afk_gemm_set_mfma() refuses it in the default build.
#ifdef AFK_PROBES
#define AFK_MFMA_SHAPES_NT 3
#define AFK_MFMA_SHAPES_NN 3
#define AFK_MFMA_SHAPES_TN 3
#else
#define AFK_MFMA_SHAPES_NT 2   // 16x16x32 wins or ties on every NT shape of the step (+1.6 .. +9.0 % by the medians)
#define AFK_MFMA_SHAPES_NN 1   // 16x16x32 ties at best, and is slower by the medians on the two dgrads the step runs on this kernel
#define AFK_MFMA_SHAPES_TN 1   // 16x16x32 loses the encoder weight gradients by 15 - 18 %
#endif

// 256x256 ping-pong kernel (gemm256.hip)
int afk_launch_gemm256(const GemmArgs& p, int mf, hipStream_t st);   // mf = 32 | 16: MFMA shape
int afk_launch_gemm256p(const GemmArgs& p, hipStream_t st);  // persistent tile loop (tools/probes/gemm256p.hip)
int afk_launch_gemm256q(const GemmArgs& p, hipStream_t st);  // persistent tile loop, next tile's prologue ahead of the epilogue stores (tools/probes/gemm256q.hip)
// 256x256, K-step 32, eight free-running waves, ten-slot LDS ring (gemm256f8.hip); mode 1 = no-DMA timing probe
int afk_launch_gemm256f8(const GemmArgs& p, int mode, hipStream_t st);
// 256x256 four-wave kernel, 128x128 per wave, accumulators in AGPRs (gemm256w4.hip)
int afk_launch_gemm256w4(const GemmArgs& p, int mode, hipStream_t st);  // mode 1 / 2: timing probes (no DMA / no DMA + no fragment reads)
// transposed-operand variants (gemm256t.hip): NN (trans_a = 0) and TN (trans_a = 1); B is reduction-major in both
int afk_launch_gemm256t(const GemmArgs& p, int trans_a, int mf, hipStream_t st);
