"""References, error bounds and case tables of everything the model runs before the first transformer layer and around the KV cache: the log-mel
front end (csrc/logmel.hip), the conv stem's data movement (im2col / col2im / weight permutation / AvgPool), the embedding gather and scatter, the
placeholder scan, the transposes, the KV-cache append, the fp32 -> bf16 cast and rotary_time (csrc/elementwise.hip).  Plain torch / numpy, no kernel
calls: importable on the CPU (tests/test_frontend_ref_cpu.py holds every reference to something independent).

DATA MOVEMENT is exact to the bit: each reference below is the definition written with padding and slicing, and the GPU module compares int16 views.
Where a kernel adds (col2im: at most two bf16 terms in fp32; AvgPool: two; the weight-gradient accumulate: two; embed_scatter_bwd: a run of rows in row
order, then the old value) the reference does the same fp32 additions in the same order and rounds once, so it is bit-exact too.

ROTARY_TIME  y0 = x0 c0 - x1 s0, y1 = x1 c1 + x0 s1 in fp32 (two products, one sum, fused or not: 3 e (|x0 c| + |x1 s|), e = 2^-24), one bf16 rounding:
_norm_ref.round_bound of that.

LOG-MEL  logmel_ref is the float64 pipeline; logmel_bound is the forward error of the kernel's fp32 arithmetic, per output, derived not chosen:
    re, im    a 400-term fp32 dot product against a basis STORED in fp32 (one more rounding per term) :  gamma(402) sum_n |x_n b_nk|, per frame and bin
              (the actual sum, an extra [frames, 400] x [400, 201] product in float64)
    P         re^2 + im^2 :  2 |re| e_re + e_re^2 + 2 |im| e_im + e_im^2 + 3 e P   (two squares and a sum, fused or not)
    mel       201 non-negative terms :  sum_k fb_mk e_P_k + gamma(202) mel
    log10     of max(mel, 1e-10) (max is 1-Lipschitz, so the floor at 1e-10 costs nothing; the fp32 constant 1e-10f is off by at most e relative):
              -log10(1 - e_mel / max(mel, 1e-10) - e), infinite where the error reaches the value (mel cancelled to nothing: such outputs are left out)
              + LOG10F_ULP ulp of the result for log10f itself.  LOG10F_ULP = 3: the OpenCL full-profile limit for log10 that the ROCm device library's
              log10f is built to (the HIP math documentation lists 2 ulp for it; 3 is the specified maximum, not a measurement)
    floor     mx - 8 with mx the window's maximum: the maximum of values each within its own bound moves by at most the largest bound among the values that
              can reach it; one fp32 rounding of the subtraction.  max(v, mx - 8) is 1-Lipschitz in both: an output clearly above the floor carries e_v, one
              clearly below carries e_floor, and one within e_v + e_floor of it may land on either side and carries the larger of the two
    (. + 4) / 4   one fp32 rounding of the sum; the scaling is exact.
Outputs whose bound exceeds LEFT_OUT_BOUND = 1e-2 are not compared; their share (and the near-floor share, reported beside it) must stay below
SHARE_CAP = 1 % in every case - a condition on the reference alone, asserted on the CPU.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

from tests import _norm_ref as N

BF = torch.bfloat16
E32 = N.E32
NAN = float("nan")


def past_cap(n_items):
    """does an ew_grid launch of n_items work items (256 per block, 4096 blocks at most) take a grid-stride step?"""
    return N.ew_past_cap(n_items)


def bits(t):
    """the int16 (bf16) / int32 (fp32) image of a tensor, so that -0 and NaN payloads count"""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gauss(shape, seed, sigma=1.0, dtype=BF):
    return (torch.randn(shape, generator=_gen(seed)) * sigma).to(dtype)


def int_data(shape, seed, lo=-8, hi=8):
    """small integers as bf16: every fp32 sum of a few thousand of them is exact in any order"""
    n = int(np.prod(shape))
    return N.small_int(n, seed, lo, hi).reshape(shape)


# ---------------------------------------------------------------------------------------------- conv stem
CONV1_TILE_T, CONV1_TILE_C = 62, 64
CONV1_CASES = ((8, 1), (64, 62), (64, 63), (72, 124), (128, 125), (136, 187))   # (C, T), W = 2
CONV1_W = 2
CONV2_TIN, CONV2_C, CONV2_W = (1, 2, 3, 100, 101), (8, 72), (1, 3)
CONV2_CAP_C, CONV2_CAP_W = 64, 2
IM2COL2_CAP_TIN = 43691     # Tout 21846: 2 * 21846 * 3 * 8 = 1,048,608 vectors
COL2IM2_CAP_TIN = 65537     # 2 * 65537 * 8 = 1,048,592 vectors (odd Tin: the last tap lands on Tin - 1)
WEIGHT_CASES = ((1, 1), (3, 5), (32, 64), (560, 640))   # (Co, Ci); the last: 560 * 640 * 3 = 1,075,200 elements
POOL_CASES = ((1, 8), (5, 72), (131075, 64))            # (out_rows, C); the last: 131075 * 8 = 1,048,600 vectors


def conv1_tiles(C, T):
    """(time tiles, channel blocks) of afk_im2col_conv1's grid"""
    return N.cdiv(T, CONV1_TILE_T), N.cdiv(C, CONV1_TILE_C)


def tout(Tin):
    return (Tin - 1) // 2 + 1


def im2col1(x):
    """x [W, C, T] f32 or bf16 -> col [W * T, 3 C] bf16:  col[(w, t)][kk C + c] = bf16(x[w][c][t + kk - 1]), zero outside"""
    W, C, T = x.shape
    xp = F.pad(x.to(BF), (1, 1))
    col = torch.stack([xp[:, :, kk: kk + T] for kk in range(3)], 0)      # [kk, w, c, t]
    return col.permute(1, 3, 0, 2).reshape(W * T, 3 * C).contiguous()


def im2col2(h, W, Tin, C):
    """h [W * Tin, C] -> col [W * Tout, 3 C]:  col[(w, to)][kk C + c] = h[w][2 to + kk - 1][c], zero outside (stride 2, pad 1)"""
    To = tout(Tin)
    hp = F.pad(h.reshape(W, Tin, C), (0, 0, 1, 1))                       # padded index = time + 1
    col = torch.stack([hp[:, kk: kk + 2 * To - 1: 2] for kk in range(3)], 2)   # [w, to, kk, c]
    assert col.shape == (W, To, 3, C)
    return col.reshape(W * To, 3 * C).contiguous()


def col2im2(dcol, W, Tin, C):
    """the adjoint of im2col2: dh[w][j][c] = the fp32 sum, in tap order, of the (at most two) dcol[(w, to)][kk C + c] with 2 to + kk - 1 == j, rounded once"""
    To = tout(Tin)
    d = dcol.reshape(W, To, 3, C).float()
    acc = torch.zeros((W, Tin + 2, C), dtype=torch.float32)
    for kk in range(3):
        acc[:, kk: kk + 2 * To - 1: 2] += d[:, :, kk]
    return acc[:, 1: Tin + 1].reshape(W * Tin, C).to(BF)


def weight_to_gemm(w):
    """[Co, Ci, 3] -> [Co, 3 Ci] tap-major"""
    Co, Ci, _ = w.shape
    return w.permute(0, 2, 1).reshape(Co, 3 * Ci).contiguous()


def weight_grad_from_gemm(dwp, old, accumulate):
    """[Co, 3 Ci] -> [Co, Ci, 3]; with accumulate bf16(float(old) + float(in))"""
    Co, Ci, _ = old.shape
    v = dwp.reshape(Co, 3, Ci).permute(0, 2, 1).contiguous()
    return (old.float() + v.float()).to(BF) if accumulate else v


def avgpool2_fwd(x, out_rows, C):
    x = x.reshape(out_rows, 2, C).float()
    return (0.5 * (x[:, 0] + x[:, 1])).to(BF)


def avgpool2_bwd(dy, out_rows, C):
    """every bf16(0.5 dy) is written twice"""
    return (0.5 * dy.reshape(out_rows, C).float()).to(BF).repeat_interleave(2, 0)


# ---------------------------------------------------------------------------------------------- placeholder scan, embedding
SCAN_WAVE, SCAN_CHUNK = 64, 1024
SCAN_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 131075)
SCAN_PATTERNS = ("none", "all", "first", "last", "wave_seam", "chunk_seam", "random_0.01", "random_0.5")
AUDIO_ID = 7


def scan_chunks(n):
    return N.cdiv(n, SCAN_CHUNK)


def scan_ids(n, pattern, seed=0):
    """int64 ids [n] with AUDIO_ID where the pattern puts a placeholder (a seam run is cut to the length of the ids), other ids elsewhere"""
    g = _gen(seed + n)
    ids = torch.randint(AUDIO_ID + 1, 50, (n,), generator=g)
    ids[::3] = torch.randint(0, AUDIO_ID, (len(ids[::3]),), generator=g)     # ids on both sides of AUDIO_ID
    m = torch.zeros(n, dtype=torch.bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[-1] = True
    elif pattern == "wave_seam":
        m[62:66] = True
    elif pattern == "chunk_seam":
        m[1022:1026] = True
    elif pattern.startswith("random_"):
        m = torch.rand(n, generator=g) < float(pattern.split("_")[1])
    else:
        assert pattern == "none"
    ids[m] = AUDIO_ID
    assert torch.equal(ids == AUDIO_ID, m)
    return ids


def placeholder_scan(ids, audio_id):
    """(src int32: the exclusive rank of a match among the matches, -1 elsewhere; the count)"""
    m = ids.reshape(-1) == audio_id
    rank = torch.cumsum(m.long(), 0) - 1
    return torch.where(m, rank, torch.full_like(rank, -1)).to(torch.int32), int(m.sum())


def embed_scatter_fwd(ids, src, embed, audio):
    """out[i] = audio[src[i]] where src[i] >= 0, else embed[ids[i]]"""
    ids = ids.reshape(-1)
    out = embed[ids].clone()
    if src is not None:
        m = src >= 0
        out[m] = audio[src[m].long()]
    return out


def embed_scatter_bwd(ids, src, dout, d_embed_old, n_audio):
    """the kernel's stated contract: d_audio[src[i]] = dout[i] on placeholder rows; every id that occurs on a text row gets
    bf16(float(old) + s), s the fp32 sum of its rows' dout taken SEQUENTIALLY in row order from 0; rows of d_embed whose id never occurs keep their bits.
    -> (d_embed, d_audio); either input may be None (d_embed_old None: no d_embed wanted)"""
    ids = ids.reshape(-1)
    n, H = dout.shape
    text = torch.ones(n, dtype=torch.bool) if src is None else src < 0
    d_audio = None
    if src is not None and n_audio is not None:
        d_audio = torch.zeros((n_audio, H), dtype=BF)
        d_audio[src[~text].long()] = dout[~text]
    if d_embed_old is None:
        return None, d_audio
    rows = text.nonzero().reshape(-1)
    order = torch.sort(ids[rows], stable=True).indices
    rows = rows[order]
    sid = ids[rows]
    head = torch.ones_like(sid, dtype=torch.bool)
    head[1:] = sid[1:] != sid[:-1]
    first = torch.cummax(torch.where(head, torch.arange(len(sid)), torch.zeros_like(sid)), 0).values
    occ = torch.arange(len(sid)) - first                                  # 0 for the first row of an id, 1 for its second, ...
    acc = torch.zeros(d_embed_old.shape, dtype=torch.float32)
    by_occ = torch.sort(occ, stable=True)
    bounds = torch.searchsorted(by_occ.values, torch.arange(int(occ.max()) + 2 if len(occ) else 1))
    for k in range(len(bounds) - 1):
        sel = by_occ.indices[bounds[k]: bounds[k + 1]]
        acc[sid[sel]] = acc[sid[sel]] + dout[rows[sel]].float()           # one fp32 addition per id and step: the sequential sum
    out = d_embed_old.clone()
    touched = torch.unique(sid)
    out[touched] = (d_embed_old[touched].float() + acc[touched]).to(BF)
    return out, d_audio


def gather_rows(x, rows):
    return x[rows].clone()


def scatter_rows(src, rows, M):
    out = torch.zeros((M, src.shape[1]), dtype=src.dtype)
    out[rows] = src
    return out


EMBED_H = (8, 64, 3584)
EMBED_SMALL_N, EMBED_BIG_N, EMBED_ONE_ID_N = 37, 131075, 5000


# ---------------------------------------------------------------------------------------------- transposes, KV append, cast
TRANSPOSE_CASES = ((1, 8), (63, 8), (64, 64), (65, 72), (100, 200), (129, 136))
HEADS_CASES = ((1, 1, 1, 64, 64), (2, 100, 3, 64, 128), (2, 65, 2, 128, 128))     # (B, S, H, D, spad)
KV_CASES = ((1, 1, 1, 64), (3, 1, 2, 128), (2, 5, 4, 64), (2, 2052, 2, 128))      # (B, n, Hkv, D); the last: 2 * 2052 * 256 = 1,050,624 elements
KV_STARTS = (0, 7)
CAST_N = (1, 1000, 1048579)


def pad64(n):
    return (n + 63) // 64 * 64


def transpose_tiles(R, C, rpad=None):
    rpad = pad64(R) if rpad is None else rpad
    return N.cdiv(C, 64) * N.cdiv(rpad, 64)


def transpose(x, rpad=None):
    """x [R, C] -> [C, rpad], columns >= R zero"""
    R, C = x.shape
    rpad = pad64(R) if rpad is None else rpad
    out = torch.zeros((C, rpad), dtype=x.dtype)
    out[:, :R] = x.t()
    return out


def transpose_heads(x, B, S, H, D, spad):
    """x [B * S, ld], element (b, s, h, d) at row b S + s, column h D + d -> [B, H, D, spad], zero padded"""
    out = torch.zeros((B, H, D, spad), dtype=x.dtype)
    out[..., :S] = x[:, : H * D].reshape(B, S, H, D).permute(0, 2, 3, 1)
    return out


def kv_append(Kc, Vt, qkv, k_col0, start, B, n, Hkv, D):
    """Kc [B, Smax, Hkv D], Vt [B, Hkv, D, Spad], qkv [B n, ld]:  Kc[b, start + i, :] = qkv[b n + i, k_col0 : k_col0 + nk],
    Vt[b, h, d, start + i] = qkv[b n + i, k_col0 + nk + h D + d]; everything else keeps its bits"""
    nk = Hkv * D
    Kc, Vt = Kc.clone(), Vt.clone()
    for b in range(B):
        for i in range(n):
            row = qkv[b * n + i]
            Kc[b, start + i, :] = row[k_col0: k_col0 + nk]
            Vt[b, :, :, start + i] = row[k_col0 + nk: k_col0 + 2 * nk].reshape(Hkv, D)
    return Kc, Vt


def cast_input(n, seed=3):
    """fp32 [n]: gaussian, with (cycled over the front of it) +-0, subnormals, exact bf16 ties that round down to even and up to even, values that round
    up into the next binade, the largest finite fp32 (rounds to inf), +-inf and NaN"""
    x = torch.randn(n, generator=_gen(seed))
    k = min(n, len(CAST_SPECIAL))
    x[:k] = (CAST_SPECIAL if n >= len(CAST_SPECIAL) else CAST_SPECIAL[ROUNDING_SPECIAL_AT:])[:k]
    return x


def _f32(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


# 1 + 2^-8 (tie, down to even), 1 + 3 * 2^-8 (tie, up to even), the same negative, 2 - 2^-8 (tie, up into the next binade), the fp32 below 2 (up into the
# next binade), one fp32 step above and below a tie
ROUNDING_SPECIAL = _f32([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3FFF8000, 0x3FFFFFFF, 0x3F808001, 0x3F807FFF])
# +-0, the smallest and largest subnormals, the largest finite values (round to inf), a tie at the top (to inf), +-inf, NaN
ROUNDING_SPECIAL_AT = 12
CAST_SPECIAL = torch.cat([_f32([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F800000,
                                0xFF800000, 0x7FC00000]), ROUNDING_SPECIAL])
assert len(CAST_SPECIAL) - len(ROUNDING_SPECIAL) == ROUNDING_SPECIAL_AT


def conv1_input(W, C, T, seed, dtype):
    """gaussian [W, C, T]; the fp32 form carries ROUNDING_SPECIAL at its front (as much of it as fits)"""
    x = torch.randn((W, C, T), generator=_gen(seed))
    if dtype == torch.float32:
        k = min(x.numel(), len(ROUNDING_SPECIAL))
        x.view(-1)[:k] = ROUNDING_SPECIAL[:k]
        return x
    return x.to(BF)


def pool_input(out_rows, C, seed):
    """gaussian bf16 [2 out_rows, C] whose first pair of rows holds, cycling over the columns: 1 and 1 + 2^-7 (mean 1 + 2^-8: a tie, down to even),
    1 + 2^-7 and 1 + 2^-6 (mean 1 + 3 * 2^-8: a tie, up to even), x and -x"""
    x = gauss((2 * out_rows, C), seed)
    a = torch.tensor([1.0, 1.0 + 2.0 ** -7, 1.7109375, -0.0])
    b = torch.tensor([1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -1.7109375, 0.0])
    idx = torch.arange(C) % 4
    x[0], x[1] = a[idx].to(BF), b[idx].to(BF)
    assert torch.equal(x[0].float(), a[idx]) and torch.equal(x[1].float(), b[idx])
    return x


# ---------------------------------------------------------------------------------------------- rotary_time
ROTARY_CASES = ((1, 2, 2), (3, 128, 0), (5, 128, 52), (5, 128, 128), (16400, 128, 52))   # (rows, E, R); the last: 16400 * 64 = 1,049,600 pairs


def rotary_time_ref(x, cos, sin, backward=False):
    """interleaved-pair rotation of the first R columns by per-(row, column) angles, float64: (value, bound).  backward = the transposed rotation"""
    X, Cs, Sn = x.double(), cos.double(), sin.double()
    rows, E = X.shape
    R = Cs.shape[-1]
    out, bound = X.clone(), torch.zeros_like(X)
    if R:
        x0, x1 = X[:, 0:R:2], X[:, 1:R:2]
        c0, c1, s0, s1 = Cs[:, 0::2], Cs[:, 1::2], Sn[:, 0::2], Sn[:, 1::2]
        if not backward:
            y0, y1 = x0 * c0 - x1 * s0, x1 * c1 + x0 * s1
            e0, e1 = (x0 * c0).abs() + (x1 * s0).abs(), (x1 * c1).abs() + (x0 * s1).abs()
        else:
            y0, y1 = x0 * c0 + x1 * s1, x1 * c1 - x0 * s0
            e0, e1 = (x0 * c0).abs() + (x1 * s1).abs(), (x1 * c1).abs() + (x0 * s0).abs()
        out[:, 0:R:2], out[:, 1:R:2] = y0, y1
        bound[:, 0:R:2], bound[:, 1:R:2] = N.round_bound(y0, 3 * E32 * e0), N.round_bound(y1, 3 * E32 * e1)
    return out, bound


def rotary_formula(x, cos, sin):
    """the float64 formula of the model file as tests/test_ops_gpu.py::test_rotary_time states it (differentiable)"""
    R = cos.shape[-1]
    xx = x.double()
    rot, rest = xx[:, :R], xx[:, R:]
    pr = rot.reshape(x.shape[0], -1, 2)
    half = torch.stack((-pr[..., 1], pr[..., 0]), -1).flatten(-2)
    return torch.cat((rot * cos.double() + half * sin.double(), rest), -1)


# ---------------------------------------------------------------------------------------------- log-mel
N_FFT, HOP, N_BINS, FRAME_BLOCK = 400, 160, 201, 32
LOG10F_ULP = 3
LEFT_OUT_BOUND = 1e-2
SHARE_CAP = 1e-2
LOGMEL_CASES = ((1, 480, 128), (3, 160 * 33, 128), (3, 160 * 64, 128), (3, 160 * 200, 64), (5, 264000, 128))   # (W, nsamp, n_mels)
MUTATIONS = ("symmetric_hann", "origin_off_by_one", "drop_first_frame", "batch_max")


def logmel_geometry(W, nsamp, n_mels):
    T = nsamp // HOP
    return NS(T=T, blocks=N.cdiv(T, FRAME_BLOCK), ragged=T % FRAME_BLOCK != 0, finish_items=W * n_mels * T, fstep=256 // n_mels)


@functools.lru_cache(maxsize=None)
def logmel_wave(W, nsamp, seed=0):
    """fp32 [W, nsamp], the window contents cycling through: white noise at 0.1; a 440 Hz tone at 0.3 plus noise at 0.01; noise at 1e-3 whose second
    half is silent"""
    rng = np.random.default_rng(seed + nsamp)
    t = np.arange(nsamp) / 16000.0
    wav = np.zeros((W, nsamp), np.float32)
    for w in range(W):
        kind = w % 3
        if kind == 0:
            wav[w] = 0.1 * rng.standard_normal(nsamp)
        elif kind == 1:
            wav[w] = 0.3 * np.sin(2 * np.pi * 440 * t) + 0.01 * rng.standard_normal(nsamp)
        else:
            wav[w, : nsamp // 2] = 1e-3 * rng.standard_normal(nsamp // 2)
    wav.setflags(write=False)
    return wav


@functools.lru_cache(maxsize=None)
def mel_bank(n_mels):
    """the fp32 mel bank the kernel reads, [201, n_mels]"""
    from audio_flamingo_amd.frontend import mel_filter_bank

    return mel_filter_bank(n_mels).astype(np.float32)


def _frames(wav, mutate=None):
    """float64 [W, T, 400]: reflect pad by 200, hop 160, the last of the T + 1 frames dropped"""
    W, nsamp = wav.shape
    assert nsamp >= N_FFT and nsamp % HOP == 0
    T = nsamp // HOP
    x = wav.astype(np.float64)
    if mutate == "reflect_off_by_one":          # the mirrored index one sample off: the edge sample repeated
        xp = np.pad(x, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="symmetric")
    elif mutate == "origin_off_by_one":         # the origin of the reflected index one sample off: 199 before, 201 after
        xp = np.pad(x, ((0, 0), (N_FFT // 2 - 1, N_FFT // 2 + 1)), mode="reflect")
    else:
        xp = np.pad(x, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="reflect")
    fr = np.lib.stride_tricks.sliding_window_view(xp, N_FFT, axis=1)[:, ::HOP]
    assert fr.shape == (W, T + 1, N_FFT)
    return fr[:, 1:] if mutate == "drop_first_frame" else fr[:, :T]


def _window(mutate=None):
    n = np.arange(N_FFT, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (N_FFT - 1 if mutate == "symmetric_hann" else N_FFT))


def _finish(v, batch_max=False):
    mx = v.max(axis=(0, 1, 2), keepdims=True) if batch_max else v.max(axis=(1, 2), keepdims=True)
    return (np.maximum(v, mx - 8.0) + 4.0) / 4.0, mx


def logmel_ref(wav, n_mels, mutate=None):
    """float64 [W, n_mels, T] of fp32 wav [W, nsamp].  mutate: one of MUTATIONS / "reflect_off_by_one" - the mistakes the bound must reject"""
    spec = np.fft.rfft(_frames(wav, mutate) * _window(mutate), axis=-1)
    power = spec.real ** 2 + spec.imag ** 2                                          # [W, T, 201]
    mel = power @ mel_bank(n_mels).astype(np.float64)                                # [W, T, n_mels]
    v = np.log10(np.maximum(mel, 1e-10)).transpose(0, 2, 1)
    return _finish(v, batch_max=mutate == "batch_max")[0]


@functools.lru_cache(maxsize=None)
def _basis64():
    n = np.arange(N_FFT, dtype=np.float64)
    ang = 2.0 * np.pi * np.outer(n, np.arange(N_BINS, dtype=np.float64)) / N_FFT
    win = _window()
    return win[:, None] * np.cos(ang), -win[:, None] * np.sin(ang)


def logmel_bound(wav, n_mels):
    """-> NS(ref, bound, keep, left_out, near_floor): float64 [W, n_mels, T]; keep = bound <= LEFT_OUT_BOUND; the two shares as floats"""
    fr = _frames(wav)
    cb, sb = _basis64()
    fb = mel_bank(n_mels).astype(np.float64)
    re, im = fr @ cb, fr @ sb
    e_re, e_im = N.gamma(N_FFT + 2) * (np.abs(fr) @ np.abs(cb)), N.gamma(N_FFT + 2) * (np.abs(fr) @ np.abs(sb))
    P = re * re + im * im
    e_P = 2 * np.abs(re) * e_re + e_re ** 2 + 2 * np.abs(im) * e_im + e_im ** 2 + 3 * E32 * P
    mel = P @ fb
    e_mel = e_P @ fb + N.gamma(N_BINS + 1) * mel
    arg = np.maximum(mel, 1e-10)
    rel = e_mel / arg + E32
    e_log = np.where(rel < 1.0, -np.log10(1.0 - np.where(rel < 1.0, rel, 0.0)), np.inf)
    v = np.log10(arg)
    e_ulp = LOG10F_ULP * 2 * E32 * np.abs(v)
    e_v = (e_log + e_ulp).transpose(0, 2, 1)
    e_up = (np.log10(1.0 + rel) + e_ulp).transpose(0, 2, 1)                          # the upward side alone, finite everywhere
    v = v.transpose(0, 2, 1)
    out, mx = _finish(v)
    # the window's fp32 maximum lies between max (v - e_v) and max (v + e_up)
    e_mx = np.maximum((v + e_up).max(axis=(1, 2), keepdims=True) - mx, mx - (v - e_v).max(axis=(1, 2), keepdims=True))
    floor = mx - 8.0
    e_floor = e_mx + E32 * np.abs(floor)
    gap = e_v + e_floor
    near = np.abs(v - floor) <= gap
    e_sel = np.where(v > floor + gap, e_v, np.where(v < floor - gap, e_floor, np.maximum(e_v, e_floor)))
    bound = 0.25 * (e_sel + E32 * (np.abs(np.maximum(v, floor)) + 4.0 + e_sel)) + N.TINY
    keep = bound <= LEFT_OUT_BOUND
    return NS(ref=logmel_ref(wav, n_mels), bound=bound, keep=keep, left_out=float(1.0 - keep.mean()), near_floor=float(near.mean()))


def logmel_fp32_restatement(wav, n_mels):
    """the kernel's steps as torch fp32 tensor operations on the CPU (the fp32 basis and mel bank the kernel reads, fp32 products and sums in torch's
    own order): an independent fp32 evaluation of the pipeline.  -> fp32 [W, n_mels, T]"""
    from audio_flamingo_amd.frontend import dft_basis

    cosb, sinb = dft_basis(N_BINS)
    W, nsamp = wav.shape
    T = nsamp // HOP
    xp = np.pad(wav, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="reflect")
    fr = torch.from_numpy(np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(xp, N_FFT, axis=1)[:, ::HOP][:, :T]))
    re, im = fr @ torch.from_numpy(cosb), fr @ torch.from_numpy(sinb)
    mel = (re * re + im * im) @ torch.from_numpy(mel_bank(n_mels))
    v = torch.log10(torch.clamp_min(mel, 1e-10)).permute(0, 2, 1)
    mx = v.amax(dim=(1, 2), keepdim=True)
    return ((torch.maximum(v, mx - 8.0) + 4.0) * 0.25).contiguous()


def logmel_ratio(got, b):
    """max |got - ref| / bound over the outputs that are compared"""
    err = np.abs(np.asarray(got, np.float64) - b.ref)
    return float((err / b.bound)[b.keep].max())


def error_percentiles(got, ref):
    """(median, 99.9th percentile) of |got - ref|"""
    err = np.abs(np.asarray(got, np.float64) - ref).reshape(-1)
    return float(np.median(err)), float(np.percentile(err, 99.9))
