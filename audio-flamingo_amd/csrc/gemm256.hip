// bf16 NT GEMM, 256x256x64 "ping-pong" kernel for gfx950 (the high-throughput variant of gemm.hip).
//
// Why: the 128x128 kernel needs 64 B/clk/CU of L2->LDS traffic at full MFMA rate - more than the ~56 B/clk/CU the
// L2s deliver - and tops out at ~35 % of peak.  A 256x256 tile halves the traffic per flop; the price is one
// workgroup per CU (128 KiB LDS), so latency must be hidden inside the workgroup.
//
// Structure.  8 waves: wave w -> M half wm = w>>2 (128 rows), N quarter wn = w&3 (64 cols); waves w and w+4 share a
// SIMD, so the two M-halves form two GROUPS with one wave of each on every SIMD.  The groups run the same program
// one barrier apart: while group 0 is in an MFMA segment (16 x v_mfma_f32_32x32x16_bf16 = 512 cycles of that SIMD's
// matrix pipe, s_setprio 1) group 1 is in a MEMORY segment (ds_read_b128 fragments + LDS-DMA issue) and vice versa,
// so every SIMD's matrix pipe always has an owner.  Per K-tile (64) a wave runs
//     MEM_a : read B (64 rows x 64 k = 8 frags, kept for the whole tile) + A rows 0..63 of its half (8 frags)
//     MFMA_a: 2x2 tiles x 4 k-steps                       -> output rows 0..63
//     MEM_b : read A rows 64..127 (8 frags)
//     MFMA_b: 2x2 tiles x 4 k-steps                       -> output rows 64..127
// each followed by one s_barrier (4 per K-tile).  Accumulators: 4x2 tiles x 16 = 128 VGPRs; operands 64 VGPRs.
//
// LDS: two 64 KiB buffers (tile parity), each = A image (256 rows x 128 B) + B image.  Row r stores 16-B chunk c at
// position c ^ ((r>>1)&7) (conflict-free ds_read_b128 for the 32x32x16 fragment; the permutation is applied on the
// SOURCE address of the lane-linear LDS-DMA and again on the read, guide rule 21).
// Prefetch schedule (LDS-DMA, 1 KiB per wave-instruction, 64 per K-tile = 8 per wave): rows die in two classes,
//     X = B rows + A rows {0..63, 128..191}   last read in MEM_a   -> restaged for tile t+2 inside MFMA_b(t) (6 per wave)
//     Y =          A rows {64..127, 192..255} last read in MEM_b   -> restaged for tile t+1 inside MFMA_a(t) (2 per wave)
// (the LDS-DMA pieces are slotted between MFMAs: their ~100-cycle issue cost disappears in the MFMA shadow)
// so every load has >= 4 segments (~2000 cycles) to land.  Per wave the issue order is X0 Y0 X1 | Y1 X2 | Y2 X3 ...
// and counted waits before the barriers (vmcnt 6 / 8 / 2 / 8 after MEM_a / MFMA_a / MEM_b / MFMA_b) retire exactly the
// class the NEXT segment of the other group reads (derivation in DESIGN.md §3); never vmcnt(0) in the steady state.  ds_reads are retired
// (lgkmcnt(0)) before the barrier that ends a MEM segment, so a slot is never restaged under an outstanding read.
// The last two K-tiles are peeled out of the loop (k_tile below): nothing is staged for tiles >= T, and the last wait of the kernel is the one that
// retires Y(T-1) after MEM_a(T-1) - a wave reaches its epilogue with no LDS-DMA in flight.
#include "gemm_common.h"

namespace {

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int ROWB = 128;              // bytes per LDS row
constexpr int OP_BYTES = 256 * ROWB;   // 32 KiB per operand image
constexpr int BUF_BYTES = 2 * OP_BYTES;
constexpr int LDS_BYTES = 2 * BUF_BYTES;  // 128 KiB

#define AFK_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define AFK_LGKMCNT0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define AFK_BARRIER()                         \
    do {                                      \
        __builtin_amdgcn_sched_barrier(0);    \
        __builtin_amdgcn_s_barrier();         \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)

// EPI: compile-time epilogue flags (gemm_common.h), -1 = runtime flags / narrow stores / split-K partials
// MF: MFMA shape (gemm_common.h): 32 = 16 x v_mfma_f32_32x32x16_bf16 per MFMA segment, 16 = 32 x v_mfma_f32_16x16x32_bf16 (same cycles, same
// fragments per segment, same 64 + 128 VGPRs); on N(0,1) operands the chip holds a higher clock on the second (profiles/gemm_mfma_shape_ab.md)
// OLDLOOP: make PROBES=1 builds only (afk_gemm_set_variant(15)) - the previous K loop, kept for the A/B of profiles/gemm_tail.md
template <int EPI, int MF, bool OLDLOOP = false>
__global__ __launch_bounds__(512, 1) void gemm_nt_bf16_k256(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;  // wm doubles as the ping-pong group
    const int hi = lane >> 5, l31 = lane & 31;

    // ---- prologue order: the first barrier waits for X0 alone, so the tile index and the six X sources come first and X0 leaves before anything else
    // is computed; Y0 and X1 follow as soon as the Y sources exist; fragment offsets and accumulator zeroing run under the loads in flight
    int tm, tn;
    gemm_tile_of_block(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int T = p.K / BK;

    // ---- LDS-DMA sources.  unit u of an operand image = rows [8u, 8u+8).  X: 6 units per wave, Y: 2 units per wave.
    // X list (48): i<32 -> B unit i ; i>=32 -> A unit (i-32 < 8 ? i-32 : i-32+8)   (A rows 0..63, 128..191)
    // Y list (16): j<8  -> A unit 8+j ; else A unit 16+j                            (A rows 64..127, 192..255)
    const bf16* xsrc[6];
    int xdst[6];
    const bf16* ysrc[2];
    int ydst[2];
    const int lrow = lane >> 3, pos = lane & 7;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int i = wave + 8 * j;
        const bool isB = i < 32;
        const int unit = isB ? i : ((i - 32) < 8 ? (i - 32) : (i - 32) + 8);
        const int rl = unit * 8 + lrow;
        const int chunk = pos ^ ((rl >> 1) & 7);
        if (isB) {
            // SWIGLU_FWD: N-tile tn = 128 gate rows [128 tn, +128) followed by the 128 up rows [I + 128 tn, +128) of the fused weight,
            // so that one workgroup holds gate AND up of the same 128 intermediate features
            const int r = (EPI == AFK_GEMM_SWIGLU_FWD) ? (rl < 128 ? tn * 128 + rl : (p.N >> 1) + tn * 128 + rl - 128) : min(n0 + rl, p.N - 1);
            xsrc[j] = p.B + (int64_t)r * p.ldb + chunk * 8;
        } else {
            const int r = min(m0 + rl, p.M - 1);
            xsrc[j] = p.A + (int64_t)r * p.lda + chunk * 8;
        }
        xdst[j] = (isB ? OP_BYTES : 0) + unit * 1024;
    }
    auto issue_x = [&](int t) {
        char* base = smem + (t & 1) * BUF_BYTES;
        const int koff = t * BK;
#pragma unroll
        for (int j = 0; j < 6; ++j)
            __builtin_amdgcn_global_load_lds((gbl_void*)(xsrc[j] + koff), (lds_void*)(base + xdst[j]), 16, 0, 0);
    };
    auto issue_y = [&](int t) {
        char* base = smem + (t & 1) * BUF_BYTES;
        const int koff = t * BK;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((gbl_void*)(ysrc[j] + koff), (lds_void*)(base + ydst[j]), 16, 0, 0);
    };
    __builtin_amdgcn_sched_barrier(0);
    issue_x(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int jj = wave + 8 * j;
        const int unit = jj < 8 ? 8 + jj : 16 + jj;
        const int rl = unit * 8 + lrow;
        const int chunk = pos ^ ((rl >> 1) & 7);
        const int r = min(m0 + rl, p.M - 1);
        ysrc[j] = p.A + (int64_t)r * p.lda + chunk * 8;
        ydst[j] = unit * 1024;
    }
    issue_y(0);
    if (T > 1) issue_x(1);   // a one-tile reduction (T = 1) stages nothing beyond its own tile
    __builtin_amdgcn_sched_barrier(0);

    // ---- fragment offsets (bytes within an operand image); the swizzle term is lane-constant
    // fragment x = 0..3 of a 32-row tile (gemm_common.h: MF = 32: k-step x; MF = 16: 16-row half x >> 1, k-step x & 1)
    int koffb[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) koffb[x] = gemm_frag_rowoff<MF>(x) * ROWB + gemm_frag_koff<MF>(x, lane);
    const int a_row0 = (wm * 128 + gemm_frag_row<MF>(lane)) * ROWB;            // + i*32*ROWB, i = 0..3 (i<2: MEM_a, i>=2: MEM_b)
    const int b_row0 = OP_BYTES + (wn * 64 + gemm_frag_row<MF>(lane)) * ROWB;  // + j*32*ROWB, j = 0..1

    GemmAcc<MF> acc;
    acc.zero();
    // all of the above runs here, under the loads in flight, not behind the barrier (afk_pin)
#pragma unroll
    for (int x = 0; x < 4; ++x) afk_pin(koffb[x]);
    int a_row0_ = a_row0, b_row0_ = b_row0;
    afk_pin(a_row0_);
    afk_pin(b_row0_);
    acc.pin();

    // ---- make X0 visible to everyone: at most Y0 (2) + X1 (6) stay in flight
    if (T > 1) AFK_VMCNT(8);
    else AFK_VMCNT(2);
    AFK_BARRIER();
    if (wm == 1) AFK_BARRIER();  // group 1 runs one segment behind group 0

    bf16x8 bf[2][4], af[2][4];
    // one LDS-DMA piece slotted behind every group of MFMAs (issue cost hides in the MFMA shadow).  A group = 128 matrix-pipe cycles:
    //   MF = 32: k-step g, 2 x 2 blocks (4 MFMAs of 32 cycles);  MF = 16: k-step g >> 1, A block g & 1, its 2 x 4 tiles (8 MFMAs of 16 cycles)
    auto mfma_group = [&](auto acc0_, auto g_) {
        constexpr int ACC0 = decltype(acc0_)::value, g = decltype(g_)::value;
        if constexpr (MF == 32) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc.mma(ACC0 + i, j, bf[j][g], af[i][g]);
        } else {
            constexpr int s = g >> 1, i = g & 1;
#pragma unroll
            for (int ih = 0; ih < 2; ++ih)
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) acc.mma(2 * (ACC0 + i) + ih, jt, bf[jt >> 1][2 * (jt & 1) + s], af[i][2 * ih + s]);
        }
    };
    // half a group (64 cycles) of MFMA_b: slot q = 0..7.  MF = 32: k-step q >> 1, A block q & 1 (2 MFMAs); MF = 16: k-step q >> 2, A block (q >> 1) & 1,
    // its 16-row half q & 1 (4 MFMAs)
    auto mfma_slot = [&](auto acc0_, auto q_) {
        constexpr int ACC0 = decltype(acc0_)::value, q = decltype(q_)::value;
        if constexpr (MF == 32) {
            constexpr int s = q >> 1, i = q & 1;
            acc.mma(ACC0 + i, 0, bf[0][s], af[i][s]);
            acc.mma(ACC0 + i, 1, bf[1][s], af[i][s]);
        } else {
            constexpr int s = q >> 2, i = (q >> 1) & 1, ih = q & 1;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) acc.mma(2 * (ACC0 + i) + ih, jt, bf[jt >> 1][2 * (jt & 1) + s], af[i][2 * ih + s]);
        }
    };
    using afk_c2 = std::integral_constant<int, 2>;
#define AFK_MFMA4(ACC0, g) mfma_group(std::integral_constant<int, ACC0>{}, std::integral_constant<int, g>{})
    // One K-tile.  MODE 0 = steady state (tiles 0 .. T-3): stages Y(t+1) in MFMA_a and X(t+2) in MFMA_b, ladder 6 / 8 / 2 / 8 (header).
    // The last two tiles are peeled out of the loop: they stage nothing past tile T-1, and their waits follow from what is still in flight -
    //   MODE 1 = tile T-2: enters with Y(T-2) [2], X(T-1) [6] outstanding, in this order.
    //       after MEM_a : the other group's MEM_b(T-2) reads Y(T-2) next  -> only X(T-1) may stay out          -> vmcnt(6)   (as in the steady state)
    //       MFMA_a      : issues Y(T-1); outstanding X(T-1) [6] Y(T-1) [2] = 8: the steady vmcnt(8) asks for nothing -> no wait
    //       after MEM_b : the other group's MEM_a(T-1) reads X(T-1) next  -> only Y(T-1) may stay out          -> vmcnt(2)   (as in the steady state)
    //       MFMA_b      : X(T) does not exist: no DMA; outstanding Y(T-1) [2], nobody reads it before MEM_b(T-1)  -> no wait
    //   MODE 2 = tile T-1: enters with Y(T-1) [2] outstanding, issues nothing.
    //       after MEM_a : the other group's MEM_b(T-1) reads Y(T-1) next  -> nothing may stay out               -> vmcnt(0)
    //       MFMA_a, MEM_b, MFMA_b: nothing in flight -> no wait.  The wave reaches the epilogue with an empty vector-memory queue by construction, so
    //       no drain precedes it, and the epilogues that reuse the operand buffers (SwiGLU forward, RoPE) see no LDS-DMA behind them.
    //   T = 1: the prologue issued X0 Y0 only and left Y0 [2] out: exactly the entry state of MODE 2.  T = 2: the prologue left Y0 [2] X1 [6]: the
    //   entry state of MODE 1 at t = 0.  The barriers are those of the steady state (4 per tile), so the two groups stay one segment apart.
    //   MODE 3 (make PROBES=1 only, afk_gemm_set_variant(15)) = the previous loop: every tile a MODE 0 tile with the prefetch index clamped to T-1,
    //   i.e. the last two tiles re-load tile T-1 into slots nobody reads, and a vmcnt(0) drains them in front of the epilogue.
    auto k_tile = [&](int t, auto mode_) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_)::value;
        constexpr bool STAGE_Y = MODE != 2, STAGE_X = MODE == 0 || MODE == 3;
        const char* buf = smem + (t & 1) * BUF_BYTES;
        const int t1 = MODE == 3 ? min(t + 1, T - 1) : t + 1, t2 = MODE == 3 ? min(t + 2, T - 1) : t + 2;
        const int e1 = (t + 1) & 1, e2 = t & 1;  // destination buffer parity follows the UNclamped tile index
        const int64_t oy = (int64_t)t1 * BK, ox = (int64_t)t2 * BK;
        char* by = smem + e1 * BUF_BYTES;
        char* bx = smem + e2 * BUF_BYTES;
        // ================= MEM_a(t): B fragments (whole tile) + A rows 0..63
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) bf[j][s] = *(const bf16x8*)(buf + b_row0_ + j * 32 * ROWB + koffb[s]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 4; ++s) af[i][s] = *(const bf16x8*)(buf + a_row0_ + i * 32 * ROWB + koffb[s]);
        AFK_LGKMCNT0();
        if constexpr (MODE == 2) AFK_VMCNT(0);
        else AFK_VMCNT(6);
        AFK_BARRIER();
        // ================= MFMA_a(t) (+ Y(t+1): 2 pieces)
        __builtin_amdgcn_s_setprio(1);
        AFK_MFMA4(0, 0);
        if constexpr (STAGE_Y) {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_global_load_lds((gbl_void*)(ysrc[0] + oy), (lds_void*)(by + ydst[0]), 16, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        AFK_MFMA4(0, 1);
        if constexpr (STAGE_Y) {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_global_load_lds((gbl_void*)(ysrc[1] + oy), (lds_void*)(by + ydst[1]), 16, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        AFK_MFMA4(0, 2);
        AFK_MFMA4(0, 3);
        __builtin_amdgcn_s_setprio(0);
        if constexpr (STAGE_X) AFK_VMCNT(8);
        AFK_BARRIER();
        // ================= MEM_b(t): A rows 64..127
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 4; ++s) af[i][s] = *(const bf16x8*)(buf + a_row0_ + (i + 2) * 32 * ROWB + koffb[s]);
        AFK_LGKMCNT0();
        if constexpr (STAGE_Y) AFK_VMCNT(2);
        AFK_BARRIER();
        // ================= MFMA_b(t) (+ X(t+2): 6 pieces)
        __builtin_amdgcn_s_setprio(1);
        afk_static_for<8>([&](auto q_) {
            constexpr int piece = decltype(q_)::value;  // 0..7, pieces 0..5 carry a DMA
            mfma_slot(afk_c2{}, q_);
            if constexpr (STAGE_X && piece < 6) {
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_global_load_lds((gbl_void*)(xsrc[piece] + ox), (lds_void*)(bx + xdst[piece]), 16, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        __builtin_amdgcn_s_setprio(0);
        if constexpr (STAGE_X) AFK_VMCNT(8);
        AFK_BARRIER();
    };
    if constexpr (OLDLOOP) {   // the previous K loop (T = 1 has no prefetch to clamp: it runs as the last tile of the new one)
        const int told = T > 1 ? T : 0;
        for (int t = 0; t < told; ++t) k_tile(t, std::integral_constant<int, 3>{});
        if (T == 1) k_tile(0, std::integral_constant<int, 2>{});
        AFK_VMCNT(0);
    } else {
        for (int t = 0; t < T - 2; ++t) k_tile(t, std::integral_constant<int, 0>{});   // branch-free steady state
        if (T > 1) k_tile(T - 2, std::integral_constant<int, 1>{});
        k_tile(T - 1, std::integral_constant<int, 2>{});
    }
#undef AFK_MFMA4
    if (wm == 0) AFK_BARRIER();  // equalise barrier counts

    if constexpr (EPI == AFK_GEMM_SWIGLU_FWD) {
        // waves wn = 0, 1 hold gate columns, wn = 2, 3 the up columns of the SAME 64 features and rows: the up waves park their
        // bf16 pieces in the (now idle) operand buffers, the gate waves pick them up and write h = bf16(bf16(silu(g)) * u) beside g
        // (same arithmetic as silu_mul_fwd_kernel on the bf16-rounded GEMM results: bit-identical to the two-kernel form).
        // (l31 and hi below are the row and the 16-byte column chunk of a lane AFTER the lane-pair exchange - the same in both MFMA shapes, gemm_common.h -
        // so both waves of a pair use one piece -> (row, column) map and the exchange keeps its shape)
        typedef __attribute__((ext_vector_type(8))) __bf16 b8;
        const int I = p.N >> 1;
        const bool up = wn >= 2;
        const int feat0 = tn * 128 + (wn & 1) * 64;                 // first of this wave's 64 intermediate features
        char* xch = smem + (wm * 2 + (wn & 1)) * 16384 + lane * 16;  // piece q of the pair at + q * 1024
        b8 pc[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    // piece q = (i, j, t): row 32 i + (lane & 31), columns 32 j + 16 t + 8 (lane >> 5) + 0..7 in both MFMA shapes (gemm_lane_swap)
                    const f32x16 blk = acc.block(i, j);
                    b8 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v0, v1;
                        gemm_lane_swap<MF>(blk[8 * t + e], blk[8 * t + 4 + e], v0, v1);
                        o[e] = (bf16)(v0 * p.alpha);
                        o[4 + e] = (bf16)(v1 * p.alpha);
                    }
                    pc[(i * 2 + j) * 2 + t] = o;
                }
        if (up) {
#pragma unroll
            for (int q = 0; q < 16; ++q) *(b8*)(xch + q * 1024) = pc[q];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + wm * 128 + i * 32 + l31;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int q = (i * 2 + j) * 2 + t;
                    const int f = feat0 + j * 32 + 16 * t + 8 * hi;   // feature (= column of h) of this piece
                    if (!up) {
                        const b8 u = *(const b8*)(xch + q * 1024);
                        b8 h;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float gf = (float)pc[q][e];
                            h[e] = (bf16)(rbf(gf * sigmoid_f(gf)) * (float)u[e]);
                        }
                        if (m < p.M) *(b8*)((bf16*)p.C2 + (int64_t)m * I + f) = h;
                    }
                    if (m < p.M) *(b8*)((bf16*)p.C + (int64_t)m * p.ldc + (up ? I : 0) + f) = pc[q];
                }
        }
        return;
    }
    if constexpr (EPI >= 0 && (EPI & AFK_GEMM_ROPE) != 0) {
        // qkv projection + rotary embedding (afk_gemm_nt_bf16_rope).  A 256-column tile holds two heads of 128 columns: waves wn = 0, 1 (2, 3) own the first /
        // second 64 columns of head 0 (1) for the same rows - each wave rounds its Linear output (+ bias) to bf16, parks the 16 pieces in the idle operand
        // buffers, and after the barrier takes its partner's (wn ^ 1: the rotate-half column d +- 64 of the same row) and applies rope_kernel's arithmetic
        // (elementwise.hip, sign = +1): x1' = bf16(bf16(x1 c) + bf16(-x2 s)), x2' = bf16(bf16(x2 c) + bf16(x1 s)).  Tiles right of rope_cols (the v heads) skip
        // the exchange.  Bit-identical to the two-launch form.
        typedef __attribute__((ext_vector_type(8))) __bf16 b8;
        const bool rot = n0 < p.rope_cols;                               // block-uniform
        char* mine = smem + (wm * 4 + wn) * 16384 + lane * 16;           // piece q at + q * 1024
        const char* theirs = smem + (wm * 4 + (wn ^ 1)) * 16384 + lane * 16;
        b8 pc[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int n = n0 + wn * 64 + j * 32 + 16 * t + 8 * hi;
                    b8 bv;
                    if constexpr ((EPI & AFK_GEMM_BIAS) != 0) bv = *(const b8*)(p.bias + n);
                    const f32x16 blk = acc.block(i, j);
                    b8 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v0, v1;
                        gemm_lane_swap<MF>(blk[8 * t + e], blk[8 * t + 4 + e], v0, v1);
                        v0 *= p.alpha;
                        v1 *= p.alpha;
                        if constexpr ((EPI & AFK_GEMM_BIAS) != 0) {
                            v0 += (float)bv[e];
                            v1 += (float)bv[4 + e];
                        }
                        o[e] = (bf16)v0;
                        o[4 + e] = (bf16)v1;
                    }
                    pc[(i * 2 + j) * 2 + t] = o;
                }
        if (rot) {
#pragma unroll
            for (int q = 0; q < 16; ++q) *(b8*)(mine + q * 1024) = pc[q];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + wm * 128 + i * 32 + l31;
            const int mc = min(m, p.M - 1);
            const int64_t pr = p.rope_pos ? p.rope_pos[mc] : mc % p.rope_S;
            // lane-major tables (S % 32 == 0, no explicit positions): the 32 rows of this accumulator block are positions pr0 .. pr0 + 31 of one table block
            const bool lanes = p.rope_cos_lanes != nullptr;
            const int64_t lbase = lanes ? (((int64_t)((m0 + wm * 128 + i * 32) % p.rope_S) >> 5) * 16 * 32 + l31) * 8 : 0;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int q = (i * 2 + j) * 2 + t;
                    const int cl = wn * 64 + j * 32 + 16 * t + 8 * hi;   // column inside the tile
                    b8 o = pc[q];
                    if (rot) {
                        const int d = cl & 127;                            // column inside the head (this wave's half: d < 64 for wn even)
                        const b8 other = *(const b8*)(theirs + q * 1024);
                        const b8 c = lanes ? *(const b8*)(p.rope_cos_lanes + lbase + (d >> 3) * 256) : *(const b8*)(p.rope_cos + pr * 128 + d);
                        const b8 sn = lanes ? *(const b8*)(p.rope_sin_lanes + lbase + (d >> 3) * 256) : *(const b8*)(p.rope_sin + pr * 128 + d);
                        const float sg = (wn & 1) ? 1.f : -1.f;            // first half: x1 c - x2 s; second half: x2 c + x1 s
#pragma unroll
                        for (int e = 0; e < 8; ++e)   // rbf_strict: see common.h (fp-contract would fuse one product into the add)
                            o[e] = (bf16)(rbf_strict((float)pc[q][e] * (float)c[e]) + rbf_strict(sg * (float)other[e] * (float)sn[e]));
                    }
                    if (m < p.M) *(b8*)((bf16*)p.C + (int64_t)m * p.ldc + n0 + cl) = o;
                }
        }
        return;
    }
    // ---- epilogue: 32 x 32 blocks (gemm_common.h)
    if (AFK_GM_NOEPI(p)) return;  // -DAFK_PROBES builds only: timing probe (afk_gemm_set_variant(2 + 256 * 0x40), wrong results): the kernel without its epilogue
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) gemm_store_block32<EPI, MF>(p, m0 + wm * 128 + i * 32, n0 + wn * 64 + j * 32, lane, acc.block(i, j));
}

}  // namespace

// the epilogues of the AF3 training step get their own instantiation; anything else (SwiGLU backward, fp32 output, narrow stores) the generic one
#define AFK_EPI_LIST(X) X(0) X(AFK_GEMM_BIAS) X(AFK_GEMM_RESIDUAL) X(AFK_GEMM_BIAS | AFK_GEMM_RESIDUAL) X(AFK_GEMM_BIAS | AFK_GEMM_GELU) \
    X(AFK_GEMM_BIAS | AFK_GEMM_GELU | AFK_GEMM_RESIDUAL) X(AFK_GEMM_ACCUM) X(AFK_GEMM_SWIGLU_FWD) X(AFK_GEMM_SWIGLU_BWD) X(AFK_GEMM_ROPE) X(AFK_GEMM_ROPE | AFK_GEMM_BIAS) X(-1)

template <int MF, bool OLD = false>
static int launch_gemm256(const GemmArgs& p, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
#define AFK_SET(F)                                                                                                                           \
    if (hipFuncSetAttribute((const void*)gemm_nt_bf16_k256<(F), MF, OLD>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess) \
        return afk_set_error(AFK_ERR_LAUNCH, "gemm256: cannot reserve %d bytes of LDS", LDS_BYTES);
        AFK_EPI_LIST(AFK_SET)
#undef AFK_SET
        attr_set = true;
    }
    const int64_t nwg = (int64_t)p.ntm * p.ntn;
    const int f = (p.wide && p.splits <= 1) ? p.flags : -1;
    switch (f) {
#define AFK_CASE(F)                                                                                              \
    case (F):                                                                                                    \
        if ((F) == -1) afk_count(AFK_CNT_GEMM_GENERIC);                                                          \
        hipLaunchKernelGGL((gemm_nt_bf16_k256<(F), MF, OLD>), dim3((unsigned)nwg), dim3(512), LDS_BYTES, st, p);      \
        break;
        AFK_EPI_LIST(AFK_CASE)
#undef AFK_CASE
        default:   // an epilogue outside the list: runtime-flag instantiation
            afk_count(AFK_CNT_GEMM_GENERIC);
            hipLaunchKernelGGL((gemm_nt_bf16_k256<-1, MF, OLD>), dim3((unsigned)nwg), dim3(512), LDS_BYTES, st, p);
    }
    return AFK_OK;
}

int afk_launch_gemm256(const GemmArgs& p, int mf, hipStream_t st) {
#ifdef AFK_PROBES
    if (AFK_GM_OLDLOOP(p)) return mf == 16 ? launch_gemm256<16, true>(p, st) : launch_gemm256<32, true>(p, st);
#endif
    if constexpr ((AFK_MFMA_SHAPES_NT & 2) != 0)
        if (mf == 16) return launch_gemm256<16>(p, st);
    if constexpr ((AFK_MFMA_SHAPES_NT & 1) != 0)
        if (mf == 32) return launch_gemm256<32>(p, st);
    return afk_set_error(AFK_ERR_UNSUPPORTED, "gemm256: the %s MFMA shape of the NT kernel is built under make PROBES=1 only", mf == 16 ? "16x16x32" : "32x32x16");
}
