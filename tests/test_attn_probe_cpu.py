"""CPU: the planted-key probes of tests/_attn_probe.py can fail.  For every layout tests/test_attn_edges_gpu.py runs, every mutated reference (a range end
or the causal diagonal moved by one, a tile-edge or split-KV chunk-edge key dropped, the wrong KV head, the neighbouring sample's first key visible, the
keys behind nsplit * 4096 dropped) must differ from the true reference by at least SEP x the bar on some probed slice - on the forward rows, and on dQ
/ dK / dV for the shorter training and interval layouts - so a kernel with that bug cannot pass the GPU tests.  Also the host's choice of decode splits."""
import types

import pytest
import torch

import _attn_probe as P


def _assert_separated(case, tag, grad=False):
    assert case.mutations, f"{tag}: no mutation changes the mask"
    weak = {}
    for name in case.mutations:
        s = case.separation(name)
        if grad:
            s = min(s, case.grad_separation(name))
        if not s >= P.SEP:
            weak[name] = round(s, 2)
    assert not weak, f"{tag}: mutations closer than {P.SEP} x the bar to the truth: {weak}"


@pytest.mark.parametrize("S", P.TRAIN_S)
@pytest.mark.parametrize("D", [64, 128])
def test_training_probes_separate_every_mutation(S, D):
    for name, B, Hq, Hkv, causal, kv_len, kv_lo in P.train_layouts(S):
        case, _, _ = P.training_case(B, S, Hq, Hkv, D, causal, kv_len=kv_len, kv_lo=kv_lo, seed=S + D)
        want = {"lo+1", "hi-1", "kv head", "neighbour"} | ({"diag-1", "diag+1"} if causal else set()) | ({"lo-1"} if kv_lo else set()) | \
            {f"drop key {j}" for j in P.TILE_KEYS if j < S} | ({"hi+1"} if kv_len or not causal else set())
        if Hkv == 1:
            want.discard("kv head")
        assert want <= set(case.mutations), (name, sorted(want - set(case.mutations)))
        _assert_separated(case, f"S={S} D={D} {name}", grad=S <= 129)


@pytest.mark.parametrize("layout", P.INTERVAL_LAYOUTS, ids=lambda l: f"B{l[0]}-Sq{l[1]}-Sk{l[2]}-H{l[3]}:{l[4]}-D{l[5]}")
def test_interval_probes_separate_every_mutation(layout):
    B, Sq, Sk, Hq, Hkv, D, _, _ = layout
    case, q, k, v, kr, do = P.interval_case(B, Sq, Sk, Hq, Hkv, D, seed=Sq + Sk)
    assert bool(case.info["empty"].any()), "no empty interval"
    assert {"begin-1", "begin+1", "end-1", "end+1"} <= set(case.mutations)
    _assert_separated(case, f"interval {layout}", grad=Sq * Sk <= 200 * 300)


@pytest.mark.parametrize("G", sorted(P.DECODE_HEADS))
@pytest.mark.parametrize("D", [64, 128])
def test_decode_probes_separate_every_mutation(G, D):
    Hq, Hkv = P.DECODE_HEADS[G]
    for fused in (True, False):
        for ns in P.decode_splits(D, fused):
            for cap in ((4096, 1024) if fused else (4096,)):
                case, _, _, _ = P.decode_case(len(P.DECODE_RANGES), P.DECODE_SMAX, Hq, Hkv, D, P.DECODE_RANGES, ns, cap=cap, seed=ns)
                edges = [n for n in case.mutations if "chunk edge" in n]
                assert len(edges) == 2 * sum(len(P.decode_chunks(lo, hi, ns, cap)[2]) for lo, hi in P.DECODE_RANGES)
                assert {"lo-1", "lo+1", "hi-1", "hi+1", "from a0", "neighbour"} <= set(case.mutations)
                _assert_separated(case, f"decode G={G} D={D} ns={ns} cap={cap}")


def test_decode_long_range_probes_separate_truncation():
    """the long-range case of the GPU suite: dropping the keys behind nsplit * 4096 (the per-head kernel before its guard, ns = 1) is caught"""
    case, _, _, _ = P.decode_case(len(P.LONG_RANGES), P.LONG_SMAX, 4, 2, 128, P.LONG_RANGES, 1, seed=5)
    assert "truncated" in case.mutations
    _assert_separated(case, "decode long range ns=1")
    case, _, _, _ = P.decode_case(len(P.LONG_RANGES), P.LONG_SMAX, 4, 2, 128, P.LONG_RANGES, 2, seed=5)
    assert "truncated" not in case.mutations
    _assert_separated(case, "decode long range ns=2")


def test_decode_chunk_edges_match_the_kernel_formula():
    assert P.decode_chunks(37, 801, 8, 4096) == (32, 104, [136, 240, 344, 448, 552, 656, 760])   # ceil(769 / 8) = 97 -> 104
    assert P.decode_chunks(0, 5000, 1, 4096) == (0, 4096, [])          # the cap: one chunk of 4 096 keys, the rest is never read - refused now
    assert P.decode_chunks(5, 9, 13, 1024) == (0, 8, [8])
    assert P.decode_chunks(3, 8000, 2, 4096) == (0, 4000, [4000])


def test_host_decode_split_choice():
    """decode_forward._decode_nsplit: decode_splits while 4 096-key chunks cover the cache, ceil(spad / 4096) beyond, refused above the one-launch merge's limit;
    the workspace is sized for the same count"""
    from audio_flamingo_amd import _lib
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    m = types.SimpleNamespace(decode_splits=8, D=128, Hq=28, DECODE_CHUNK_KEYS=Mine.DECODE_CHUNK_KEYS)
    ns = lambda spad: Mine._decode_nsplit(m, spad)
    assert Mine.DECODE_CHUNK_KEYS == 4096
    assert [ns(s) for s in (64, 4096, 32768, 32832, 30274 + 2560, 40960, 126976)] == [8, 8, 8, 9, 9, 10, 31]
    with pytest.raises(_lib.AfkError, match="split merge holds at most 31"):
        ns(126976 + 64)
    m.decode_splits = 1
    assert [ns(s) for s in (1024, 4096, 4160, 8000)] == [1, 1, 2, 2]
    m.D = 64
    assert ns(62 * 4096) == 62
    with pytest.raises(_lib.AfkError):
        ns(62 * 4096 + 8)
    m._decode_nsplit = types.MethodType(Mine._decode_nsplit, m)
    aws = torch.zeros(_lib.load().afk_attn_decode_workspace_floats(1, m.Hq, m.D, 2))
    assert Mine._decode_attn_ws_check(m, aws, 1, 8000) == 2
    with pytest.raises(_lib.AfkError, match="workspace"):
        Mine._decode_attn_ws_check(m, aws, 1, 12352)


def test_decode_kernel_refuses_a_cache_its_splits_cannot_cover():
    """afk_attn_decode / _fused validate before any GPU work: spad > nsplit * 4096 is refused (the keys behind the last chunk would not be read)"""
    from audio_flamingo_amd import _lib

    buf = torch.zeros(1 << 12, dtype=torch.float32)   # host memory, never touched: validation fails first
    p = buf.data_ptr()
    D, Hq, Hkv, nk, spad = 128, 4, 2, 256, 4160
    for fn in ("afk_attn_decode", "afk_attn_decode_fused"):
        with pytest.raises(_lib.AfkError, match="spad 4160 > nsplit 1"):
            _lib.call(fn, p, Hq * D, D, p, spad * nk, nk, D, p, Hkv * D * spad, spad, p, Hq * D, D, p, 1, Hq, Hkv, D, D ** -0.5, 1, p, 0)
