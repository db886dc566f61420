// 256x256x64 ping-pong GEMM, transposed-operand variants (companion of gemm256.hip - read its header first).
//
//   NN  (dgrad):  C[M,N] = A[M,K] . Bt[K,N]        A k-contiguous,  B stored reduction-major  (dX = dY . W, W as nn.Linear stores it)
//   TN  (wgrad):  C[M,N] = At[K,M]^T . Bt[K,N]     both operands reduction-major             (dW = dY^T . X, activations as they lie)
//
// so the backward of a Linear needs NO transposed copy of anything: the W^T shadows and the activation transposes of
// round-1's first version (31 ms/step of pure HBM traffic, 15 GB of HBM) are gone.
//
// A reduction-major operand is staged as the image [64 k-rows][256 cols] (512-byte rows, LDS-DMA reads full 512-byte
// lines) and its MFMA fragment "col x 8 consecutive k" is fetched with two ds_read_b64_tr_b16 (4 k-rows x 16 cols per
// 16-lane group, lane i receives column i; rows 8hi..8hi+3 and 8hi+4..8hi+7 so that the k order matches the
// ds_read_b128 fragment of a k-contiguous operand).  16-byte chunk c of row r is stored at c ^ (((r&3)<<2)|((r>>2)&3)):
// the four rows of a tr-read block fall into four different 64-byte windows (conflict-free).
//
// Ping-pong schedule, LDS-DMA lifetime classes and the counted-vmcnt ladder are those of gemm256.hip with
//   NN: X = Bt image (32 pieces) + A rows {0..63,128..191} (16)  -> 6 per wave;  Y = A rows {64..127,192..255} -> 2 per wave
//       phases split by output rows (m halves); ladder vmcnt 6 / 8 / 2 / 8
//   TN: phases split by K (k-steps 0,1 | 2,3): X = k-rows 0..31 of both images (4 per wave), Y = k-rows 32..63 (4 per
//       wave); ladder vmcnt 4 / 8 / 4 / 8.  K need not be a multiple of 64: out-of-range k-rows are read clamped (finite
//       data) and the A fragments of the last tile are zeroed for k >= K.
#include "gemm_common.h"

namespace {

constexpr int BK = 64;
constexpr int OP_BYTES = 32768;
constexpr int BUF_BYTES = 2 * OP_BYTES;
constexpr int LDS_BYTES = 2 * BUF_BYTES;
constexpr int TROW = 512;  // bytes per row of a transposed image

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

#define AFK_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define AFK_LGKMCNT0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define AFK_BARRIER()                         \
    do {                                      \
        __builtin_amdgcn_sched_barrier(0);    \
        __builtin_amdgcn_s_barrier();         \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
#define AFK_DMA_PTR(SRCPTR, DSTPTR)                                                                       \
    do {                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        __builtin_amdgcn_global_load_lds((gbl_void*)(SRCPTR), (lds_void*)(DSTPTR), 16, 0, 0);             \
        __builtin_amdgcn_sched_barrier(0);                                                                \
    } while (0)

__device__ __forceinline__ int tswz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// fragment of a transposed image: lane -> column 32*tile32 + (lane&31), k = 16*s + 8*hi + 0..7.
// The swizzle term of a tr-read address does not depend on the k-step s (16*s leaves r&3 and (r>>2)&3 unchanged), so the
// two byte offsets of a (tile, piece) pair are lane constants: they are computed once per kernel and every read is
// "base + immediate" (s*8192 fits the 16-bit ds offset field) - no VALU in the MEM segments.
//
// 16x16x32 shape (MF = 16): lane -> column 16*tile16 + (lane&15), k = 32*s + 8*(lane>>4) + 0..7: the 16-lane group g reads k-rows 8g + 4pc + 0..3 of
// the 16 columns of its tile; the two 32-lane halves of a read touch k-rows {0..3, 8..11} and {16..19, 24..27} (+ 4 for pc = 1), whose swizzle terms
// tswz differ in bit 1 between the two groups of a half and in bits 2, 3 between the rows of a group: conflict-free (tests/test_gemm_frag_map_cpu.py).
// 32*s leaves the swizzle term unchanged as well, so the offsets stay lane constants + immediates (s*16384).
// Fragment x of a 32-column tile: MF = 32: k-step x (0..3); MF = 16: 16-column half x >> 1, k-step x & 1 - as for the k-contiguous image.
template <int MF>
__device__ __forceinline__ int tr_off(int tile, int pc, int lane) {   // tile: 32-column tile (MF = 32) or 16-column tile (MF = 16)
    const int g = lane >> 4, i = lane & 15;
    const int chunk = MF == 16 ? 2 * tile + ((i & 3) >> 1) : 4 * tile + 2 * (g & 1) + ((i & 3) >> 1);
    const int r = (MF == 16 ? 8 * g : 8 * (g >> 1)) + (i >> 2) + 4 * pc;  // + 16*s (MF = 32), + 32*s (MF = 16)
    return r * TROW + ((chunk ^ tswz(r)) << 4) + 8 * (i & 1);
}
// opaque-asm reads (common.h: the builtin form drags an s_waitcnt vmcnt(0) into the loop); every MEM segment ends with
// AFK_LGKMCNT0 + a scheduling barrier before the first MFMA, which is the wait these reads need
template <int MF, int S>
__device__ __forceinline__ bf16x8 tr_frag(uint32_t buf, int off0, int off1) {
    return afk_lds_tr_frag<S * (48 - MF) * TROW>(buf + off0, buf + off1);   // k-step S starts at k-row 16 S (MF = 32) / 32 S (MF = 16): S * (48 - MF) rows
}

// per-lane source of one LDS-DMA piece (1 KiB = 2 k-rows x 512 B) of a transposed image
struct TSrc {
    const bf16* base;  // + column offset (already clamped into the row)
    int krow;          // k-row inside the tile (0..63)
};
__device__ __forceinline__ TSrc tsrc(const bf16* mat, int unit, int col0, int ncols, int lane) {
    const int krow = 2 * unit + (lane >> 5);
    const int pos = lane & 31;
    const int chunk = pos ^ tswz(krow);
    const int col = min(col0 + chunk * 8, ncols - 8);
    TSrc s;
    s.base = mat + col;
    s.krow = krow;
    return s;
}

// EPI: compile-time epilogue flags (gemm_common.h: one small epilogue instead of every variant inlined at each store site), -1 = runtime
// MF: MFMA shape, 32 = v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16 (gemm_common.h; only fragments, MFMA calls and accumulator indexing differ)
// OLDLOOP: make PROBES=1 builds only (afk_gemm_set_variant(15)) - the previous K loop, kept for the A/B of profiles/gemm_tail.md
template <bool AT, int EPI, int MF, bool OLDLOOP = false>
__global__ __launch_bounds__(512, 1) void gemm_xt_bf16_k256(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int hi = lane >> 5, l31 = lane & 31;

    int tm, tn;
    gemm_tile_of_block(p, tm, tn);
    const int m0 = tm * 256, n0 = tn * 256;
    // split-K (blockIdx.y = split): this block reduces K-tiles [t0, t1) of its output tile; operands are re-based so that the body
    // below runs unchanged on the local reduction length KL
    int KL = p.K;
    const bf16* Abase = p.A;
    const bf16* Bbase = p.B;
    if (p.splits > 1) {
        const int tall = (p.K + BK - 1) / BK;
        const int t0 = (int)((int64_t)tall * blockIdx.y / p.splits), t1 = (int)((int64_t)tall * (blockIdx.y + 1) / p.splits);
        const int kbeg = t0 * BK;
        KL = min(p.K, t1 * BK) - kbeg;
        Abase += AT ? (int64_t)kbeg * p.lda : (int64_t)kbeg;
        Bbase += (int64_t)kbeg * p.ldb;
    }
    const int T = (KL + BK - 1) / BK;
    constexpr int NX = AT ? 4 : 6, NY = AT ? 4 : 2;

    // ------------------------------------------------------------------ LDS-DMA piece table
    // normal A image (NN only): unit = 8 rows x 128 B, chunk permutation c ^ ((r>>1)&7)
    const bf16* an_src[NX + NY];  // k-contiguous sources (advance by t*64 elements)
    TSrc tr_src[NX + NY];         // reduction-major sources (advance by t*64 rows)
    int64_t tr_ld[NX + NY];
    int dst[NX + NY];
    const bf16* tbase[NX + NY];
    auto make_piece = [&](int j) __attribute__((always_inline)) {
        const bool isx = j < NX;
        const int jj = isx ? j : j - NX;
        an_src[j] = nullptr;
        tr_src[j].base = nullptr;
        tr_src[j].krow = 0;
        tr_ld[j] = 0;
        if (AT) {
            // X: k-rows 0..31 (units 0..15) of A (jj<2) then B (jj>=2); Y: k-rows 32..63 (units 16..31) likewise
            const bool isA = jj < 2;
            const int unit = (isx ? 0 : 16) + wave + 8 * (jj & 1);
            tr_src[j] = isA ? tsrc(Abase, unit, m0, p.M, lane) : tsrc(Bbase, unit, n0, p.N, lane);
            tr_ld[j] = isA ? p.lda : p.ldb;
            dst[j] = (isA ? 0 : OP_BYTES) + unit * 1024;
        } else if (isx && jj < 4) {
            const int unit = wave + 8 * jj;  // Bt image, 32 pieces
            tr_src[j] = tsrc(Bbase, unit, n0, p.N, lane);
            tr_ld[j] = p.ldb;
            dst[j] = OP_BYTES + unit * 1024;
        } else {
            // A (k-contiguous): X (jj = 4,5) -> units {0..7, 16..23}, Y (jj = 0,1) -> units {8..15, 24..31}
            const int k = wave + 8 * (isx ? jj - 4 : jj);
            const int unit = isx ? (k < 8 ? k : k + 8) : (k < 8 ? 8 + k : 16 + k);
            const int rl = unit * 8 + (lane >> 3);
            const int chunk = (lane & 7) ^ ((rl >> 1) & 7);
            const int r = min(m0 + rl, p.M - 1);
            an_src[j] = Abase + (int64_t)r * p.lda + chunk * 8;
            dst[j] = unit * 1024;
        }
        tbase[j] = (AT || j < 4) ? tr_src[j].base + (int64_t)tr_src[j].krow * tr_ld[j] : nullptr;
    };
    // reduction-major pieces: per-lane base already at the piece's k-row, advanced per K-tile by a wave-uniform (scalar) offset - one 64-bit
    // add per DMA.  The row clamp (k-rows beyond the reduction length) only exists in a ragged LAST tile: that one takes the general form.
    // (The general form on every piece - per-lane min + 64-bit multiply, ~10 VALU between two MFMAs, eight times per K-tile - cost the TN
    // kernel ~8 % against the NT kernel: profiles/r02_gemm_probes.md §12.)
    // Prologue order: the first barrier waits for X0 alone, so only the X pieces are set up ahead of the first LDS-DMA; the Y pieces follow X0, then Y0
    // and X1 leave, and the read offsets and the accumulator zeroing run under the loads in flight.
#pragma unroll
    for (int j = 0; j < NX; ++j) make_piece(j);
    GemmAcc<MF> acc;

    const bool ragged = (KL % BK) != 0;
  // the whole pipeline twice: RAG = false (K a multiple of 64: every training shape) never clamps, RAG = true is the general form
  auto pipeline = [&](auto rag_) {
    constexpr bool RAG = decltype(rag_)::value;
    auto src_of = [&](int j, int t) -> const bf16* {
        const bool tr = AT || j < 4;  // compile-time after unrolling
        if (tr) {
            if constexpr (RAG) {
                const int row = min(t * BK + tr_src[j].krow, KL - 1);
                return tr_src[j].base + (int64_t)row * tr_ld[j];
            } else {
                return tbase[j] + (int64_t)t * BK * tr_ld[j];
            }
        }
        return an_src[j] + (int64_t)t * BK;
    };
    auto issue = [&](int j, int t_src, int parity) { AFK_DMA_PTR(src_of(j, t_src), smem + parity * BUF_BYTES + dst[j]); };

    // ------------------------------------------------------------------ prologue: X0 | Y0 X1 (a one-tile reduction, T = 1, stages no X1)
#pragma unroll
    for (int j = 0; j < NX; ++j) issue(j, 0, 0);
#pragma unroll
    for (int j = 0; j < NY; ++j) make_piece(NX + j);
#pragma unroll
    for (int j = 0; j < NY; ++j) issue(NX + j, 0, 0);
    if (T > 1) {
#pragma unroll
        for (int j = 0; j < NX; ++j) issue(j, 1, 1);
    }
    acc.zero();

    // lane-constant tr-read offsets: B tiles wn*2+j, A tiles wm*4+i (TN); MF = 16: [tile][h][pc] = 16-column half h of the 32-column tile
    constexpr int NH = MF == 16 ? 2 : 1;
    int tob[2][NH][2], toa[4][NH][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) tob[j][h][pc] = OP_BYTES + tr_off<MF>((wn * 2 + j) * NH + h, pc, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) toa[i][h][pc] = AT ? tr_off<MF>((wm * 4 + i) * NH + h, pc, lane) : 0;
    // fragment x = 0..3 of a 32-column tile, k-steps [KS0, KS0 + NKS) of the tile: MF = 32 -> k-step x; MF = 16 -> half x >> 1, k-step x & 1
    // (TN reads half a tile per phase: x = 0, 1 with KS0 = the phase's first k-step - MF = 32: k-step KS0 + x; MF = 16: half x, k-step KS0)
    auto tr_read = [&](uint32_t lbuf, const int (&to)[NH][2], auto x_, auto ks0_) {
        constexpr int x = decltype(x_)::value, ks0 = decltype(ks0_)::value;
        if constexpr (MF == 32) return tr_frag<MF, ks0 + x>(lbuf, to[0][0], to[0][1]);
        else if constexpr (AT) return tr_frag<MF, ks0>(lbuf, to[x][0], to[x][1]);
        else return tr_frag<MF, (x & 1)>(lbuf, to[x >> 1][0], to[x >> 1][1]);
    };
    // fragment offsets for the k-contiguous A image (NN), as in gemm256.hip
    int koffb[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) koffb[x] = gemm_frag_rowoff<MF>(x) * 128 + gemm_frag_koff<MF>(x, lane);
    int a_row0 = (wm * 128 + gemm_frag_row<MF>(lane)) * 128;
    // all of the above runs here, under the loads in flight, not behind the barrier (afk_pin)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) afk_pin(tob[j][h][pc]);
    if constexpr (AT) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int h = 0; h < NH; ++h)
#pragma unroll
                for (int pc = 0; pc < 2; ++pc) afk_pin(toa[i][h][pc]);
    } else {
#pragma unroll
        for (int x = 0; x < 4; ++x) afk_pin(koffb[x]);
        afk_pin(a_row0);
    }
    acc.pin();

    // X0 visible to everyone: at most Y0 (NY) + X1 (NX) stay in flight
    if (T > 1) AFK_VMCNT(8);
    else if (AT) AFK_VMCNT(4);
    else AFK_VMCNT(2);
    AFK_BARRIER();
    if (wm == 1) AFK_BARRIER();

    bf16x8 bf[2][4], af[AT ? 4 : 2][AT ? 2 : 4];
    const uint32_t lds0 = afk_lds_addr(smem);
    // One K-tile, as k_tile of gemm256.hip (the derivation is there; NX / NY = 6 / 2 for NN, 4 / 4 for TN, issue order X0 Y0 X1 | Y1 X2 | ...):
    //   MODE 0 = steady state, tiles 0 .. T-3: Y(t+1) staged in the first MFMA segment, X(t+2) in the second; waits NX / 8 / NY / 8
    //   MODE 1 = tile T-2: enters with Y(T-2) [NY] X(T-1) [NX] out.  After the first MEM segment Y(T-2) must be in -> vmcnt(NX); the first MFMA segment
    //            issues Y(T-1): 8 out, no wait; after the second MEM segment X(T-1) must be in -> vmcnt(NY); the second MFMA segment stages nothing
    //            (X(T) does not exist) and waits for nothing
    //   MODE 2 = tile T-1: enters with Y(T-1) [NY] out and stages nothing.  After the first MEM segment -> vmcnt(0); no wait after that: the epilogue
    //            starts with nothing in flight.  T = 1 enters here from the prologue (Y0 out), T = 2 enters MODE 1 (Y0 X1 out).
    //   MODE 3 (make PROBES=1 only, afk_gemm_set_variant(15)) = the previous loop: MODE 0 with the prefetch index clamped to T-1, drained by a vmcnt(0)
    // The ragged last tile of TN (kvalid < 64) is tile T-1 in every mode: its zeroing of the A fragments and the clamped source rows (src_of) are untouched.
    auto k_tile = [&](int t, auto mode_) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_)::value;
        constexpr bool STAGE_Y = MODE != 2, STAGE_X = MODE == 0 || MODE == 3;
        const char* buf = smem + (t & 1) * BUF_BYTES;
        const uint32_t lbuf = lds0 + (t & 1) * BUF_BYTES;
        const int t1 = MODE == 3 ? min(t + 1, T - 1) : t + 1, t2 = MODE == 3 ? min(t + 2, T - 1) : t + 2;
        const int e1 = (t + 1) & 1, e2 = t & 1;
        if constexpr (!AT) {
            // ================= NN  MEM_a: Bt fragments (whole tile) + A rows 0..63
#pragma unroll
            for (int j = 0; j < 2; ++j)
                afk_static_for<4>([&](auto x_) { bf[j][decltype(x_)::value] = tr_read(lbuf, tob[j], x_, std::integral_constant<int, 0>{}); });
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int s = 0; s < 4; ++s) af[i][s] = *(const bf16x8*)(buf + a_row0 + i * 32 * 128 + koffb[s]);
            AFK_LGKMCNT0();
            if constexpr (MODE == 2) AFK_VMCNT(0);
            else AFK_VMCNT(6);
            AFK_BARRIER();
            // ================= MFMA_a (+ Y(t+1))
            __builtin_amdgcn_s_setprio(1);
            afk_static_for<4>([&](auto g_) {   // groups of 128 matrix-pipe cycles, as in gemm256.hip
                constexpr int g = decltype(g_)::value;
                if constexpr (MF == 32) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc.mma(i, j, bf[j][g], af[i][g]);
                } else {
                    constexpr int s = g >> 1, i = g & 1;
#pragma unroll
                    for (int ih = 0; ih < 2; ++ih)
#pragma unroll
                        for (int jt = 0; jt < 4; ++jt) acc.mma(2 * i + ih, jt, bf[jt >> 1][2 * (jt & 1) + s], af[i][2 * ih + s]);
                }
                if constexpr (STAGE_Y && g < 2) issue(NX + g, t1, e1);
            });
            __builtin_amdgcn_s_setprio(0);
            if constexpr (STAGE_X) AFK_VMCNT(8);
            AFK_BARRIER();
            // ================= MEM_b: A rows 64..127
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int s = 0; s < 4; ++s) af[i][s] = *(const bf16x8*)(buf + a_row0 + (i + 2) * 32 * 128 + koffb[s]);
            AFK_LGKMCNT0();
            if constexpr (STAGE_Y) AFK_VMCNT(2);
            AFK_BARRIER();
            // ================= MFMA_b (+ X(t+2))
            __builtin_amdgcn_s_setprio(1);
            afk_static_for<8>([&](auto q_) {   // slots of 64 matrix-pipe cycles
                constexpr int piece = decltype(q_)::value;
                if constexpr (MF == 32) {
                    constexpr int s = piece >> 1, i = piece & 1;
                    acc.mma(2 + i, 0, bf[0][s], af[i][s]);
                    acc.mma(2 + i, 1, bf[1][s], af[i][s]);
                } else {
                    constexpr int s = piece >> 2, i = (piece >> 1) & 1, ih = piece & 1;
#pragma unroll
                    for (int jt = 0; jt < 4; ++jt) acc.mma(2 * (2 + i) + ih, jt, bf[jt >> 1][2 * (jt & 1) + s], af[i][2 * ih + s]);
                }
                if constexpr (STAGE_X && piece < 6) issue(piece, t2, e2);
            });
            __builtin_amdgcn_s_setprio(0);
            if constexpr (STAGE_X) AFK_VMCNT(8);
            AFK_BARRIER();
        } else {
            const int kvalid = KL - t * BK;  // < 64 only on a ragged last tile
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                // ================= TN  MEM: fragments of k-steps {2ph, 2ph+1} of both images
                // (first k-step of phase ph: 2 ph of four 16-wide, ph of two 32-wide)
                afk_static_for<2>([&](auto x_) {
                    constexpr int x = decltype(x_)::value;
                    constexpr int KS = MF == 16 ? 1 : 2;
                    if (ph == 0) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) bf[j][x] = tr_read(lbuf, tob[j], x_, std::integral_constant<int, 0>{});
#pragma unroll
                        for (int i = 0; i < 4; ++i) af[i][x] = tr_read(lbuf, toa[i], x_, std::integral_constant<int, 0>{});
                    } else {
#pragma unroll
                        for (int j = 0; j < 2; ++j) bf[j][x] = tr_read(lbuf, tob[j], x_, std::integral_constant<int, KS>{});
#pragma unroll
                        for (int i = 0; i < 4; ++i) af[i][x] = tr_read(lbuf, toa[i], x_, std::integral_constant<int, KS>{});
                    }
                });
                AFK_LGKMCNT0();
                if (RAG && kvalid < BK) {  // block-uniform, ragged last tile only (the RAG = false pipeline has no such tile): zero the A contribution of k >= K
#pragma unroll
                    for (int s = 0; s < 2; ++s)   // fragment s of the phase: MF = 32: k-step 2 ph + s; MF = 16: column half s of k-step ph
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const bool dead = (MF == 16 ? 32 * ph + 8 * (lane >> 4) : 16 * (2 * ph + s) + 8 * hi) + e >= kvalid;
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (dead) af[i][s][e] = (bf16)0.f;
                        }
                }
                // after MEM of phase 0: Y(t) must be in (X(t+1) may stay out); of phase 1: X(t+1) must be in (Y(t+1) may stay out)
                if constexpr (MODE == 2) {
                    if (ph == 0) AFK_VMCNT(0);
                } else {
                    AFK_VMCNT(4);
                }
                AFK_BARRIER();
                // ================= MFMA (+ Y(t+1) in phase 0, X(t+2) in phase 1: 4 pieces each)
                __builtin_amdgcn_s_setprio(1);
                afk_static_for<8>([&](auto q_) {   // slots of 64 matrix-pipe cycles
                    constexpr int piece = decltype(q_)::value;  // 0..7, even pieces carry a DMA
                    if constexpr (MF == 32) {
                        constexpr int s = piece >> 2, i = piece & 3;
                        acc.mma(i, 0, bf[0][s], af[i][s]);
                        acc.mma(i, 1, bf[1][s], af[i][s]);
                    } else {
                        constexpr int i = piece >> 1, ih = piece & 1;   // A block i, its 16-column half ih, against the 4 B tiles
#pragma unroll
                        for (int jt = 0; jt < 4; ++jt) acc.mma(2 * i + ih, jt, bf[jt >> 1][jt & 1], af[i][ih]);
                    }
                    if constexpr ((piece & 1) == 0) {
                        if (ph == 0) {
                            if constexpr (STAGE_Y) issue(NX + (piece >> 1), t1, e1);
                        } else {
                            if constexpr (STAGE_X) issue(piece >> 1, t2, e2);
                        }
                    }
                });
                __builtin_amdgcn_s_setprio(0);
                if constexpr (STAGE_X) AFK_VMCNT(8);
                AFK_BARRIER();
            }
        }
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
    if (wm == 0) AFK_BARRIER();
  };
    if (ragged) pipeline(std::true_type{});
    else pipeline(std::false_type{});

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) gemm_store_block32<EPI, MF>(p, m0 + wm * 128 + i * 32, n0 + wn * 64 + j * 32, lane, acc.block(i, j));
}

}  // namespace

// weight gradients write or accumulate plain bf16 (flags 0 / ACCUM); the generic instantiation serves split-K partials and the rest
#define AFK_EPI_LIST(X) X(0) X(AFK_GEMM_ACCUM) X(-2) X(-1)

template <bool AT, int MF, bool OLD = false>
static int launch_gemm256t(const GemmArgs& p, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
#define AFK_SET(F)                                                                                                                              \
    if (hipFuncSetAttribute((const void*)gemm_xt_bf16_k256<AT, (F), MF, OLD>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess) \
        return afk_set_error(AFK_ERR_LAUNCH, "gemm256t: cannot reserve %d bytes of LDS", LDS_BYTES);
        AFK_EPI_LIST(AFK_SET)
#undef AFK_SET
        attr_set = true;
    }
    const int64_t nwg = (int64_t)p.ntm * p.ntn;
    const unsigned ns = (unsigned)(p.splits > 1 ? p.splits : 1);
    const int f = p.splits > 1 ? -2 : (p.wide ? p.flags : -1);  // -2: split-K partial sums (the fold kernel applies the epilogue)
    const dim3 grid((unsigned)nwg, ns);
    switch (f) {
#define AFK_CASE(F)                                                                                        \
    case (F):                                                                                              \
        if ((F) == -1) afk_count(AFK_CNT_GEMM_GENERIC);                                                    \
        hipLaunchKernelGGL((gemm_xt_bf16_k256<AT, (F), MF, OLD>), grid, dim3(512), LDS_BYTES, st, p);           \
        break;
        AFK_EPI_LIST(AFK_CASE)
#undef AFK_CASE
        default:   // an epilogue outside the list: runtime-flag instantiation
            afk_count(AFK_CNT_GEMM_GENERIC);
            hipLaunchKernelGGL((gemm_xt_bf16_k256<AT, -1, MF, OLD>), grid, dim3(512), LDS_BYTES, st, p);
    }
    return AFK_OK;
}

int afk_launch_gemm256t(const GemmArgs& p, int trans_a, int mf, hipStream_t st) {
#ifdef AFK_PROBES
    if (AFK_GM_OLDLOOP(p))
        return trans_a ? (mf == 16 ? launch_gemm256t<true, 16, true>(p, st) : launch_gemm256t<true, 32, true>(p, st))
                       : (mf == 16 ? launch_gemm256t<false, 16, true>(p, st) : launch_gemm256t<false, 32, true>(p, st));
#endif
    if (trans_a) {
        if constexpr ((AFK_MFMA_SHAPES_TN & 2) != 0)
            if (mf == 16) return launch_gemm256t<true, 16>(p, st);
        if constexpr ((AFK_MFMA_SHAPES_TN & 1) != 0)
            if (mf == 32) return launch_gemm256t<true, 32>(p, st);
    } else {
        if constexpr ((AFK_MFMA_SHAPES_NN & 2) != 0)
            if (mf == 16) return launch_gemm256t<false, 16>(p, st);
        if constexpr ((AFK_MFMA_SHAPES_NN & 1) != 0)
            if (mf == 32) return launch_gemm256t<false, 32>(p, st);
    }
    return afk_set_error(AFK_ERR_UNSUPPORTED, "gemm256t: the %s MFMA shape of the %s kernel is built under make PROBES=1 only", mf == 16 ? "16x16x32" : "32x32x16",
                         trans_a ? "TN" : "NN");
}
