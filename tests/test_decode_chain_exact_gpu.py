"""GPU: the decode-chain Linears (csrc/decode_chain.hip) bit for bit against integer references, at the edges of their guards.

tests/_chain_ref.py draws operands on which every rounding point of the kernels is exact ({-1, 0, 1} inputs, weights and cos / sin tables, rows +-2^e in front of a
norm), so the expected output is integer arithmetic and every launch - whatever its form, K split, MFMA shape or number of sequences - must equal it with
torch.equal; the forms are then bit-equal to each other for free.  tests/test_decode_chain_ref_cpu.py shows on the reference alone that a dropped K block, a doubled
k element, a row, position or statistic of the wrong sequence and swapped halves each change it.  The only comparisons with a tolerance: SwiGLU outputs at 2^-7
relative to fp64 g sigmoid(g) u (two bf16 roundings, 2^-9 each, doubled for the fp32 sigmoid; exact zeros where g or u is 0), and the gaussian statistic cases
(all of a row's energy in its last elements / behind k = 4096, where a statistic that misses them gives rstd ~ 1000) at the bars of tests/test_ops_gpu.py.

Outputs, caches and stride padding are filled with a sentinel; everything outside the written slots must keep it.  The shapes come from R.grid(): every M of
1 .. 32 with two K's per entry, K = 8 .. 4160 (one block with seven idle slices, 9 and 17 blocks over 8 slices, the second pass of the statistics), the smallest N /
I / head shapes each guard admits, one N = 32768 for the forms that switch on the row count; every second case strided (ldx, ldw as a column slice, ld_res,
ld_out, ldq, k_bs, vt_bs, an inner cache slot).  Each shape was read against the kernel that takes it before it was launched."""
import pytest
import torch

from tests import _chain_ref as R

pytestmark = pytest.mark.gpu

BF, F64 = torch.bfloat16, torch.float64
SENT = 768.0                     # 3 x 2^8: a bf16 / fp32 / int32 value, and none an integer case writes (|v| <= 256 there)
EPS = R.EPS
SMAX = 6                         # cache slots
SWIGLU = (0.0, 2.0 ** -7)        # (atol, rtol)
BAR, BAR_GU = (3e-2, 2e-2), (3e-2, 3e-2)   # the project's bars (tests/test_ops_gpu.py), the gaussian cases only
KNOBS = ["", "S=1,1,1,1,1", "S=2,2,2,2,2 R=4,4,4,4,4", "S=8,8,8,8,8", "S=4,4,4,4,4 R=4,4,4,4,4"]   # as test_decode_chain_kernels_vs_standalone_sequence sets them
FORMS = ["", "MFMA=0", "MFMA=1", "MFMA=0 S=1,1,1,1,1", "MFMA=0 S=2,2,2,2,2", "MFMA=0 S=8,8,8,8,8"]   # M <= 8: the form chosen by M, dot product, matrix pipe


def _set(monkeypatch, knobs):
    """the knobs that are read per launch"""
    for k in ("S", "R", "MFMA", "KIL", "MFMA_NARROW"):
        monkeypatch.delenv("AFK_CHAIN_" + k, raising=False)
    for kv in knobs.split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv("AFK_CHAIN_" + k, v)


def _full(shape, dev, dtype=BF):
    return torch.full(shape, SENT, device=dev, dtype=dtype)


def _vec(t, dev, dtype=BF):
    v = t.to(dev).to(dtype).contiguous()
    assert torch.equal(v.double(), t.to(dev).double()), "an operand is not a value of its format"
    return v


def _rows(t, dev, pad=0, off=0):
    """t [R, C] as the columns off .. off + C of a sentinel-filled [R, C + pad] bf16 buffer"""
    t = t.to(dev)
    buf = _full((t.shape[0], t.shape[1] + pad), dev)
    view = buf[:, off:off + t.shape[1]]
    view.copy_(t)
    assert torch.equal(view.double(), t.double()), "an operand is not a bf16 value"
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0
    return view


class Want:
    """what a buffer must hold after the launch: the sentinel everywhere but in the written slots"""

    def __init__(self, shape, dev):
        self.exp = torch.full(shape, SENT, device=dev, dtype=F64)
        self.mask = torch.zeros(shape, device=dev, dtype=torch.bool)

    def put(self, index, value):
        self.exp[index] = value
        self.mask[index] = True
        return self

    def hold(self, tag, got, tol=None):
        g = got.double().reshape(self.exp.shape)
        if tol is None:
            ok = torch.equal(g, self.exp)
            bad = (g != self.exp) if not ok else None
        else:   # inside the written slots |got - ref| <= atol + rtol |ref|, outside them the sentinel bit for bit
            bound = torch.where(self.mask, tol[0] + tol[1] * self.exp.abs(), torch.zeros_like(self.exp))
            bad = ~((g - self.exp).abs() <= bound)
            ok = not bool(bad.any())
        if not ok:
            at = bad.nonzero()[0].tolist()
            i = tuple(at)
            raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ ({int((bad & ~self.mask).sum())} outside the written slots); "
                                 f"first at {at}: got {float(g[i])}, want {float(self.exp[i])}")


def _quantise(c, dev):
    """FP8 codes and row scales of c.W through decode_w8.quantize_rows -> (Q8, its dequantisation in fp64)"""
    from audio_flamingo_amd import decode_w8

    q = decode_w8.quantize_rows(c.W.to(dev).to(BF).contiguous())
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(dev)
    return q, (lut[q.codes.int()] * q.scale[:, None]).double()


def _prepare(entry, c, strided, dev, w8=False, tol=None, x_dev=None, ss=None):
    """buffers, expected contents and the argument list of one case -> go(tag): launch into fresh sentinel-filled outputs, hold them to the reference, return them.
    x_dev: the input rows as another launch left them (a device view);  ss: (ss_part, parts) of the launch that wrote them"""
    from audio_flamingo_amd import _lib, ops

    st = ops._stream()
    kind, single = R.kind_of(entry), entry in R.SINGLE
    name = "afk_decode_chain_" + entry + ("_w8" if w8 else "")
    M, K, N = c.M, c.K, c.N
    keep = []                                      # every tensor whose address goes into the argument list lives as long as go() does
    pad = 8 if strided else 0
    opad = 2 if strided else 0                     # scalar stores (and 32-bit ones of linear_residual_norm_batched): any even leading dimension
    assert K % (16 if w8 else 8) == 0 and (single or 1 <= M <= 32) and (not single or M == 1)
    if w8:
        q8, deq = _quantise(c, dev)
        assert torch.equal(deq, c.W.to(dev)), "the FP8 copy must be lossless"
        qpad = 16 if strided else 0
        codes = torch.full((N, K + qpad), 0x7E, device=dev, dtype=torch.uint8)[:, qpad:]   # a column slice of a wider matrix
        codes.copy_(q8.codes)
        assert codes.data_ptr() % 16 == 0 and codes.stride(0) % 16 == 0
        wa = (codes.data_ptr(), codes.stride(0), q8.scale.data_ptr())
        keep += [codes, q8]
    else:
        W = _rows(c.W, dev, pad, pad)                 # a column slice of a wider matrix
        wa = (W.data_ptr(), W.stride(0))
        keep.append(W)
    x = x_dev if x_dev is not None else _rows(c.x, dev, 0 if single else pad)
    assert torch.equal(x.double(), c.x.to(dev)) and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0
    ldx = x.stride(0)
    ref = R.reference(c, dev)
    nw = _vec(c.nw, dev) if c.norm else None
    ssa = (ss[0].data_ptr(), ss[1]) if ss is not None else (None, 0)
    keep += [x, nw, ss]

    if kind == "qkv":
        Hq, Hkv, D = c.heads
        nq, nk = Hq * D, Hkv * D
        assert N == nq + 2 * nk and D % 16 == 0
        spad, start = (10, 3) if strided else (8, 2)          # an inner slot: 0 < start < SMAX - 1, start < spad
        wide = strided and not single
        ldq, k_bs, vt_bs = nq + (8 if wide else 0), SMAX * nk + (24 if wide else 0), nk * spad + (40 if wide else 0)
        bias, cos, sin = _vec(c.bias, dev), _vec(c.cos, dev), _vec(c.sin, dev)
        pos = c.pos.to(dev).to(torch.int32)
        assert int(pos.max()) < cos.shape[0] and cos.shape[1] == D
        start_t = torch.tensor([start], device=dev, dtype=torch.int32)
        wq = Want((M, ldq), dev).put((slice(None), slice(0, nq)), ref["q"])
        wk = Want((M, k_bs), dev).put((slice(None), slice(start * nk, (start + 1) * nk)), ref["k"])                 # Kc[m][start][nk]
        wv = Want((M, vt_bs), dev).put((slice(None), torch.arange(nk, device=dev) * spad + start), ref["v"])       # Vt[m][row][start]
        rope = (bias.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr())
        keep += [bias, cos, sin, pos, start_t]

        def go(tag):
            q, Kc, Vt = _full((M, ldq), dev), _full((M, k_bs), dev), _full((M, vt_bs), dev)
            tail = (spad, start_t.data_ptr(), Hq, Hkv, D)
            if single:
                args = (x.data_ptr(), nw.data_ptr(), EPS, *wa, K, *rope, q.data_ptr(), Kc.data_ptr(), Vt.data_ptr(), *tail, st)
            elif c.norm:
                args = (x.data_ptr(), ldx, M, nw.data_ptr(), EPS, *wa, K, *rope, q.data_ptr(), ldq, Kc.data_ptr(), k_bs, Vt.data_ptr(), vt_bs, *tail, *ssa, st)
            else:
                args = (x.data_ptr(), ldx, M, *wa, K, *rope, q.data_ptr(), ldq, Kc.data_ptr(), k_bs, Vt.data_ptr(), vt_bs, *tail, st)
            _lib.call(name, *args)
            wq.hold(f"{tag} q", q, tol), wk.hold(f"{tag} k cache", Kc, tol), wv.hold(f"{tag} v cache", Vt, tol)
            return dict(q=q, Kc=Kc, Vt=Vt)
        go.keep = keep
        return go

    if kind == "lin":
        with_ss, with_n2 = entry == "linear_residual_ss_batched", entry == "linear_residual_norm_batched"
        res = _rows(c.res, dev, 0 if single else pad)
        ld_out = N + (0 if single else 8 if (with_ss and strided) else opad)   # the ss form's rows feed a launch that wants ldx % 8 == 0
        wo = Want((M, ld_out), dev).put((slice(None), slice(0, N)), ref["out"])
        if with_ss:   # [groups of eight sequences][8][N / 16 blocks]; the slots behind M are written, with zeros
            parts, NG = N // 16, 1 if M <= 8 else 2 if M <= 16 else 4
            want_ss = torch.zeros((NG * 8, parts), device=dev, dtype=F64)
            want_ss[:M] = ref["ss"]
        if with_n2:
            n2w, ld_h = _vec(c.n2w, dev), N + opad
            wh = Want((M, ld_h), dev).put((slice(None), slice(0, N)), ref["h"])
            cnt = torch.zeros(1, device=dev, dtype=torch.int32)

        def go(tag):
            out = _full((M, ld_out), dev)
            got = dict(out=out)
            if single:
                _lib.call(name, x.data_ptr(), *wa, N, K, res.data_ptr(), out.data_ptr(), st)
            elif with_ss:
                got["ss"] = _full((NG * 8, parts), dev, torch.float32)
                _lib.call(name, x.data_ptr(), ldx, M, *wa, N, K, res.data_ptr(), res.stride(0), out.data_ptr(), ld_out, got["ss"].data_ptr(), st)
                if tol is None:
                    assert torch.equal(got["ss"].double(), want_ss), f"{tag}: ss_part is not the integer sum of squares per block (zeros behind M)"
            elif with_n2:
                got["h"] = _full((M, ld_h), dev)
                _lib.call(name, x.data_ptr(), ldx, M, *wa, N, K, res.data_ptr(), res.stride(0), out.data_ptr(), ld_out, n2w.data_ptr(), EPS, got["h"].data_ptr(), ld_h,
                          cnt.data_ptr(), st)
                wh.hold(f"{tag} normalised rows", got["h"], tol)
                assert int(cnt) == 0, f"{tag}: the hand-over counter must reset itself"
            else:
                _lib.call(name, x.data_ptr(), ldx, M, *wa, N, K, res.data_ptr(), res.stride(0), out.data_ptr(), ld_out, st)
            wo.hold(f"{tag} out", out, tol)
            return got
        go.keep = keep
        return go

    if kind == "gu":
        I = c.I
        ld_act = I + (0 if single else opad)
        wa_ = Want((M, ld_act), dev).put((slice(None), slice(0, I)), ref["act"])
        gtol = tol if tol is not None else SWIGLU

        def go(tag):
            act = _full((M, ld_act), dev)
            if single:
                _lib.call(name, x.data_ptr(), nw.data_ptr(), EPS, *wa, I, K, act.data_ptr(), st)
            elif c.norm:
                _lib.call(name, x.data_ptr(), ldx, M, nw.data_ptr(), EPS, *wa, I, K, act.data_ptr(), ld_act, *ssa, st)
            else:
                _lib.call(name, x.data_ptr(), ldx, M, *wa, I, K, act.data_ptr(), ld_act, st)
            wa_.hold(f"{tag} act", act, gtol)
            return dict(act=act)
        go.keep = keep
        return go

    ld = N + (0 if single else opad)
    wl = Want((M, ld), dev).put((slice(None), slice(0, N)), ref["logits"])

    def go(tag):
        logits = _full((M, ld), dev, torch.float32)
        got = dict(logits=logits)
        if single:
            for with_logits in (True, False):   # plain greedy decoding writes no logits row: the partial pairs alone
                pv, pi = _full((N // 8,), dev, torch.float32), _full((N // 8,), dev, torch.int32)
                _lib.call(name, x.data_ptr(), nw.data_ptr(), EPS, *wa, N, K, logits.data_ptr() if with_logits else None, pv.data_ptr(), pi.data_ptr(), st)
                if tol is None:   # integer logits tie constantly: (max, FIRST index of the max) per eight rows
                    assert torch.equal(pv.double(), ref["part_val"][0]), f"{tag}: part_val"
                    assert torch.equal(pi.long(), ref["part_idx"][0]), f"{tag}: part_idx is not the first index of the group's maximum"
            got.update(pv=pv, pi=pi)
        elif c.norm:
            _lib.call(name, x.data_ptr(), ldx, M, nw.data_ptr(), EPS, *wa, N, K, logits.data_ptr(), ld, *ssa, st)
        else:
            _lib.call(name, x.data_ptr(), ldx, M, *wa, N, K, logits.data_ptr(), ld, st)
        wl.hold(f"{tag} logits", logits, tol)
        return got
    go.keep = keep
    return go


_PREPARED = {}


def _cases(entry, M, dev, w8=False):
    """the prepared cases of (entry, M): operands, references and expected buffers are built once per case and left unchanged.  The single-sequence cases
    (M = None) are shared by the knob sets of their test; the others live as long as the test that asked for them"""
    make = lambda: [(f"{entry}{'_w8' if w8 else ''} M={c.M} K={c.K} N={c.N}{' strided' if s else ''}", c, _prepare(entry, c, s, dev, w8=w8))
                    for c, s in R.grid(entry, M) if not w8 or c.K % 16 == 0]
    if M is not None:
        return make()
    if (entry, w8) not in _PREPARED:
        _PREPARED[entry, w8] = make()
    return _PREPARED[entry, w8]


def _select(tag, pv, pi, want, dev, strided):
    """afk_decode_select_greedy on the partial pairs: the first index of the global maximum, the state advanced, the token's embedding row fetched"""
    from audio_flamingo_amd import _lib, ops

    V, H = 8 * pv.numel(), 8
    emb = _full((V, H + (4 if strided else 0)), dev)[:, :H]
    emb.copy_(((torch.arange(V, device=dev)[:, None] * 7 + torch.arange(H, device=dev)[None]) % 251).to(BF))
    nxt = torch.full((1,), -1, device=dev, dtype=torch.int64)
    toks = torch.full((8,), -1, device=dev, dtype=torch.int64)
    state = torch.tensor([3, 41, 40, 37], device=dev, dtype=torch.int32)
    x0 = _full((H + 8,), dev)
    _lib.call("afk_decode_select_greedy", pv.data_ptr(), pi.data_ptr(), pv.numel(), nxt.data_ptr(), toks.data_ptr(), 5 - 40, state.data_ptr(), emb.data_ptr(), emb.stride(0), H,
              x0.data_ptr(), ops._stream())
    assert int(nxt) == want, f"{tag}: token {int(nxt)}, the first index of the maximum is {want}"
    assert toks.tolist() == [-1] * 5 + [want, -1, -1] and state.tolist() == [3, 42, 41, 38], tag
    assert torch.equal(x0[:H], emb[want]) and torch.equal(x0[H:], _full((8,), dev)), tag


# ------------------------------------------------------------------------------------------------ one sequence: gemv_chain_kernel, bf16 and FP8 weights
@pytest.mark.parametrize("knobs", KNOBS)
def test_single_sequence_entries_equal_the_integer_reference(dev, knobs, monkeypatch):
    """afk_decode_chain_{qkv, linear_residual, gate_up, lm_head} and their _w8 forms (K % 16 == 0; codes through decode_w8.quantize_rows, lossless here) at
    K = 8 .. 4160: less than one vector per lane, one chunk + a one-vector tail, 8.1 chunks (the second pass of the row statistic), every S / R form;
    part_val / part_idx and afk_decode_select_greedy on constantly tying integer logits"""
    _set(monkeypatch, knobs)
    n = 0
    for entry in R.SINGLE:
        for w8 in (False, True):
            for i, (tag, c, go) in enumerate(_cases(entry, None, dev, w8)):
                got = go(f"{tag} [{knobs}]")
                n += 1
                if entry == "lm_head":
                    want = int(R.reference(c, dev)["token"][0])
                    _select(tag, got["pv"], got["pi"], want, dev, i % 2 == 1)
    assert n == (4 * 7 + 1) + (4 * 5 + 1)   # every K of K_DOT and the row-count switch of the lm_head; FP8: the multiples of 16


def test_select_greedy_first_index_of_the_maximum(dev):
    """the select launch alone on synthetic partial pairs: 1 pair, fewer than a wave, around one round of 1024 threads, more than one round trip of 8 x 1024"""
    for nparts in (1, 7, 1023, 1025, 9000):
        g = torch.Generator().manual_seed(nparts)
        pv = torch.randint(-3, 4, (nparts,), generator=g).float().to(dev)            # ties everywhere
        pi = (8 * torch.arange(nparts) + torch.randint(0, 8, (nparts,), generator=g)).to(torch.int32).to(dev)
        want = int(pi[(pv == pv.max()).nonzero()[0]])
        _select(f"nparts={nparts}", pv, pi, want, dev, nparts % 2 == 1)


# ------------------------------------------------------------------------------------------------ 1 .. 32 sequences, inputs already normalised
@pytest.mark.parametrize("M", R.M_ALL)
@pytest.mark.parametrize("entry", R.PLAIN_BATCHED)
def test_plain_batched_entries_equal_the_integer_reference(dev, entry, M, monkeypatch):
    """M <= 8: gemv_chain_batched_kernel (MB = 2 / 4 / 8, every S) and gemv_chain_mfma_kernel (AFK_CHAIN_MFMA unset / 0 / 1; shapes only the dot-product form
    takes stay on it); M > 8: gemv_chain_mfma_ng_kernel with two / four column groups.  Each against the integer reference, hence all forms bit-equal"""
    for tag, c, go in _cases(entry, M, dev):
        for form in (FORMS if M <= 8 else [""]):
            _set(monkeypatch, form)
            go(f"{tag} [{form}]")


@pytest.mark.parametrize("entry", R.PLAIN_BATCHED)
def test_slice_ownership_and_narrow_forms(dev, entry, monkeypatch):
    """AFK_CHAIN_KIL=0 (one contiguous K slice per wave: 9 blocks over 8 slices leave three waves without a block, 17 blocks give an uneven last slice) and
    AFK_CHAIN_MFMA_NARROW=16,16 (16-row groups x 16 slices), once per entry"""
    kind = R.kind_of(entry)
    kw = dict(qkv=dict(heads=(2, 1, 32)), lin=dict(N=160), gu=dict(I=48), head=dict(N=1056))[kind]
    for i, (M, K) in enumerate(((5, 576), (8, 1088), (3, 64))):
        c = R.make(kind, M, K, 50 + i, **kw)
        go = _prepare(entry, c, i == 1, dev)
        for form in ("MFMA=1 KIL=0", "MFMA=1 MFMA_NARROW=16,16", "MFMA=1 KIL=0 MFMA_NARROW=16,16"):
            _set(monkeypatch, form)
            go(f"{entry} M={M} K={K} [{form}]")


# ------------------------------------------------------------------------------------------------ RMSNorm in the prologue / behind the Linear (matrix pipe only)
@pytest.mark.parametrize("M", R.M_ALL)
@pytest.mark.parametrize("entry", R.NORM_BATCHED)
def test_norm_in_prologue_entries_equal_the_integer_reference(dev, entry, M):
    """rows +-s_m with s_m a power of two that differs between neighbours: a sequence normalised with another sequence's statistic is off by a power of two"""
    for tag, c, go in _cases(entry, M, dev):
        go(tag)


@pytest.mark.parametrize("M", R.M_ALL[:7])
def test_linear_residual_norm_equals_the_integer_reference(dev, M):
    """Linear + residual + the RMSNorm that follows: the residual stream and the normalised rows, three launches on one counter"""
    for tag, c, go in _cases("linear_residual_norm_batched", M, dev):
        for rep in range(3):
            go(f"{tag} launch {rep}")


@pytest.mark.parametrize("M", R.M_ALL)
def test_ss_form_and_its_consumers(dev, M):
    """afk_decode_chain_linear_residual_ss_batched: out and ss_part (per block of 16 columns, exactly the integer sum of squares, zeros behind M).  Where the rows
    it leaves are +-2^(m % 5), the next Linear takes them as they lie, with ss_part and without: the same integer reference, hence the same bits"""
    for tag, c, go in _cases("linear_residual_ss_batched", M, dev):
        got = go(tag)
        if not c.target:
            continue
        rows = got["out"][:, :c.N]
        for entry, kw in (("qkv_norm_batched", dict(heads=(2, 1, 32))), ("gate_up_norm_batched", dict(I=16)), ("lm_head_norm_batched", dict(N=32))):
            cc = R.make(R.kind_of(entry), M, c.N, c.seed + 500, norm=True, rows=c.out_rows, s_e0=0, **kw)
            for ss in (None, (got["ss"], c.N // 16)):
                _prepare(entry, cc, False, dev, x_dev=rows, ss=ss)(f"{tag} -> {entry} {'with' if ss else 'without'} ss_part")


# ------------------------------------------------------------------------------------------------ what the integer form cannot see: the reach of the statistics
def _gaussian_cases(entry, w8=False):
    """(case, tolerance) x 2: the row's energy in its last 8 elements; K = 4160 with the energy in [4096, 4160) - the second pass of the single-sequence statistic,
    the c >= T CPT loop of the batched one.  linear_residual_norm_batched takes its statistic over the N <= 4096 OUTPUT columns: the last 8 of 160, the last 8 of 4096"""
    kind = R.kind_of(entry)
    tol = BAR_GU if kind == "gu" else BAR
    if entry == "linear_residual_norm_batched":
        return [(R.gaussian("lin", M, 64, 70 + M, (0, 64), norm=False, N=N, n2=True), tol) for M, N in ((5, 160), (8, 4096))]
    kw = dict(qkv=dict(heads=(2, 1, 32)), gu=dict(I=16), head=dict(N=32))[kind]
    K1 = (528 if w8 else 520) if entry in R.SINGLE else 576   # FP8: K % 16 == 0, the energy in the second half of the last lane's vector
    Ms = (1,) if entry in R.SINGLE else (5, 12)
    return [(R.gaussian(kind, M, K, 80 + M, win, **kw), tol) for M in Ms for K, win in ((K1, (K1 - 8, K1)), (4160, (4096, 4160)))]


@pytest.mark.parametrize("entry", R.NORM_IN_PROLOGUE + ("linear_residual_norm_batched",))
def test_statistics_reach_the_end_of_the_row(dev, entry):
    for c, tol in _gaussian_cases(entry):
        tag = f"{entry} gaussian M={c.M} K={c.K} N={c.N}"
        _prepare(entry, c, False, dev, tol=tol)(tag)
    if entry in R.SINGLE:   # the FP8 form, on the weights its codes stand for
        for c, tol in _gaussian_cases(entry, w8=True):
            c.W = _quantise(c, dev)[1].cpu()
            _prepare(entry, c, False, dev, w8=True, tol=tol)(f"{entry}_w8 gaussian K={c.K} N={c.N}")
