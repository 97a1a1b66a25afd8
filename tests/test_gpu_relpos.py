"""tc_attn_temporal_rel on the MI355X (csrc/attention_temporal_rel.hip): temporal attention with relative position and / or a
causal mask, and the two UNet kwargs that reach it.

Against the fp32 statement of the attention (relpos_cases.RelEmuOps) at the bound tests/test_gpu_temporal_long.py holds the
long-clip kernel to against the same kind of statement (rel-L2 <= 8e-3: the roundings are the same, the per-distance sums
add one bf16 rounding of the same order); exact properties of the mask, of the clamp ends and of the padding; refusals
without a launch; the torch.ops binding bit-equal to ctypes; the tiny UNet of every variant against the reference's golden
(tests/golden/make_relpos_golden.py) and under hipGraph replay.
"""
import ctypes as C
import hashlib

import pytest
import torch

import relpos_cases as rc
from conftest import load_golden, rel_l2
from tooncrafter_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV, BF16 = "cuda", torch.bfloat16


def _with_backend(backend, fn):
    prev = ops.set_backend(backend)
    try:
        return fn()
    finally:
        ops.set_backend(prev)


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def emu():
    return rc.RelEmuOps()


@pytest.fixture(scope="module")
def golden():
    return load_golden("unet_relpos_tiny.npz")


def rnd(*shape, seed=0, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def tables(max_rel, seed):
    """Entries at standard deviation 0.5: both relative terms are of the size of the plain ones."""
    return rnd(2 * max_rel + 1, 64, seed=seed, scale=0.5), rnd(2 * max_rel + 1, 64, seed=seed + 1, scale=0.5)


def _raw(qkv, out, rel_k, rel_v, b, t, hw, heads, max_rel, causal, scale=0.125):
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    p = _lib.TcAttnTemporalRelParams(qkv=ptr(qkv), out=ptr(out), rel_k=ptr(rel_k), rel_v=ptr(rel_v), b=b, t=t, hw=hw,
                                     heads=heads, max_rel=max_rel, causal=causal, scale=scale)
    return _lib.load().tc_attn_temporal_rel(C.byref(p), None)


# ------------------------------------------------------------------------------------------------ against the statement
_TL = [(1, 4), (4, 4), (6, 4), (16, 16), (16, 4), (17, 16), (32, 16), (33, 8), (40, 4), (64, 16), (64, 64), (24, 32)]
# hw, heads and b rotate over the cases; hw 7 with one head (7 | 14 waves: a tail wave in the 4-wave blocks) comes up three times
_CASES = [(t, L, [7, 40][i % 2], [1, 5][(i // 2) % 2], 1 + (i // 4 + i) % 2) for i, (t, L) in enumerate(_TL)]


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("t,max_rel,hw,heads,b", _CASES)
def test_rel_attention_vs_statement(hip, emu, t, max_rel, hw, heads, b, causal):
    qkv = rnd(b * t * hw, 3 * heads * 64, seed=t * 1000 + max_rel * 10 + causal)
    rk, rv = tables(max_rel, seed=t + max_rel)
    kw = dict(b=b, t=t, hw=hw, heads=heads, max_rel=max_rel, causal=causal)
    o = hip.attention_temporal_rel(qkv, rk, rv, **kw)
    r = emu.attention_temporal_rel(qkv, rk, rv, **kw)
    assert o.shape == r.shape and o.dtype == BF16 and torch.isfinite(o).all()
    e = rel_l2(o, r)
    # the same inputs without the tables: the relative terms must matter at this bound, or the case checks nothing
    d = rel_l2(emu.attention_temporal_rel(qkv, None, None, **kw), r)
    print(f"rel temporal attn b{b} t{t} L{max_rel} hw{hw} h{heads} causal{causal}: rel-L2 {e:.3e} (tables move the output by {d:.3e})")
    assert d > 0.1
    assert e <= 8e-3


@pytest.mark.parametrize("t,hw,heads,b", [(4, 7, 1, 2), (16, 40, 5, 1), (33, 7, 5, 2), (64, 40, 1, 1)])
def test_mask_only_vs_statement(hip, emu, t, hw, heads, b):
    qkv = rnd(b * t * hw, 3 * heads * 64, seed=300 + t)
    kw = dict(b=b, t=t, hw=hw, heads=heads, max_rel=0, causal=1)
    e = rel_l2(hip.attention_temporal_rel(qkv, None, None, **kw), emu.attention_temporal_rel(qkv, None, None, **kw))
    print(f"causal temporal attn without tables b{b} t{t} hw{hw} h{heads}: rel-L2 {e:.3e}")
    assert e <= 8e-3


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("t", [4, 16, 17, 32, 33, 64])
def test_no_tables_no_mask_is_plain_temporal_attention(hip, t):
    """(1) With both tables NULL and causal = 0 the kernel is tc_attn_temporal: the same core, so the same bits, at 17 .. 64
    frames; up to 16 frames tc_attn_temporal is the VALU kernel with fp32 softmax weights, and the operator bound holds."""
    b, hw, heads = 2, 7, 5
    qkv = rnd(b * t * hw, 3 * heads * 64, seed=40 + t)
    o = hip.attention_temporal_rel(qkv, None, None, b=b, t=t, hw=hw, heads=heads, max_rel=0, causal=0)
    p = hip.attention_temporal(qkv, b=b, t=t, hw=hw, heads=heads)
    if t > 16:
        assert torch.equal(o, p), f"{int((o != p).sum())} of {o.numel()} outputs differ"
    else:
        assert rel_l2(o, p) <= 8e-3


@pytest.mark.parametrize("t,max_rel", [(1, 4), (6, 4), (16, 16), (40, 4), (64, 64)])
def test_query_0_under_the_causal_mask_sees_only_itself(hip, t, max_rel):
    """(2) Frame 0 attends to key 0 alone: its weight is exactly 1 and the distance is 0, so the output rows of frame 0 are
    bf16(v_0 + Rv[L]), and v_0 itself without tables."""
    b, hw, heads = 2, 7, 5
    c = heads * 64
    qkv = rnd(b * t * hw, 3 * c, seed=60 + t)
    rk, rv = tables(max_rel, seed=7)
    o = hip.attention_temporal_rel(qkv, rk, rv, b=b, t=t, hw=hw, heads=heads, max_rel=max_rel, causal=1).reshape(b, t, hw, heads, 64)
    v0 = qkv.reshape(b, t, hw, 3, heads, 64)[:, 0, :, 2]
    assert torch.equal(o[:, 0], (v0.float() + rv[max_rel].float()).to(BF16))
    o = hip.attention_temporal_rel(qkv, None, None, b=b, t=t, hw=hw, heads=heads, max_rel=0, causal=1).reshape(b, t, hw, heads, 64)
    assert torch.equal(o[:, 0], v0)


@pytest.mark.parametrize("t", [16, 40])
@pytest.mark.parametrize("with_tables", [False, True])
def test_causal_output_does_not_depend_on_the_future(hip, t, with_tables):
    """(3) Other finite values in the frames after f0 = t / 2: the outputs of frames <= f0 keep their bits."""
    b, hw, heads, L = 2, 7, 5, 8
    c = heads * 64
    f0 = t // 2
    rk, rv = tables(L, seed=9) if with_tables else (None, None)
    qkv = rnd(b * t * hw, 3 * c, seed=80 + t)
    other = qkv.clone().reshape(b, t, hw, 3 * c)
    other[:, f0 + 1:] = rnd(b, t - f0 - 1, hw, 3 * c, seed=81 + t, scale=3.0)
    kw = dict(b=b, t=t, hw=hw, heads=heads, max_rel=L, causal=1)
    o1 = hip.attention_temporal_rel(qkv, rk, rv, **kw).reshape(b, t, hw, c)
    o2 = hip.attention_temporal_rel(other.reshape(b * t * hw, 3 * c), rk, rv, **kw).reshape(b, t, hw, c)
    assert torch.equal(o1[:, :f0 + 1], o2[:, :f0 + 1])
    assert not torch.equal(o1[:, f0 + 1:], o2[:, f0 + 1:])
    nc = hip.attention_temporal_rel(other.reshape(b * t * hw, 3 * c), rk, rv, **dict(kw, causal=0)).reshape(b, t, hw, c)
    assert not torch.equal(o1[:, :f0 + 1], nc[:, :f0 + 1])               # without the mask the future is seen


@pytest.mark.parametrize("t", [6, 17, 33])
@pytest.mark.parametrize("causal", [0, 1])
def test_clip_boundaries_and_padding(hip, t, causal):
    """(4) b = 2: the first clip's output is what it is alone; with every row behind the first clip NaN (the second clip
    and a margin: what a padded key or query slot would read) it is finite and unchanged; sentinel rows in front of and
    behind the output stay."""
    hw, heads, L, margin = 7, 5, 4, 64
    c = heads * 64
    n = t * hw
    rk, rv = tables(L, seed=13)
    x = torch.cat([rnd(n, 3 * c, seed=70 + t), rnd(n, 3 * c, seed=90 + t, scale=30.0)])
    kw = dict(t=t, hw=hw, heads=heads, max_rel=L, causal=causal)
    both = hip.attention_temporal_rel(x, rk, rv, b=2, **kw)
    alone = hip.attention_temporal_rel(x[:n].clone(), rk, rv, b=1, **kw)
    assert torch.equal(both[:n], alone) and torch.isfinite(both).all()
    buf = torch.full((2 * n + margin, 3 * c), float("nan"), dtype=BF16, device=DEV)
    buf[:n] = x[:n]
    out = torch.full((margin + n + margin, c), 7.0, dtype=BF16, device=DEV)
    assert _raw(buf, out[margin:], rk, rv, 1, t, hw, heads, L, causal) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[margin:margin + n], alone)
    assert bool((out[:margin] == 7.0).all()) and bool((out[margin + n:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ refusals, bindings
def test_refusals_launch_nothing(hip):
    qkv = rnd(65 * 8, 3 * 64, seed=3)
    out = torch.full((65 * 8, 64), 7.0, dtype=BF16, device=DEV)
    rk, rv = tables(4, seed=1)
    big = rnd(131, 64, seed=2)
    assert _raw(qkv, out, rk, rv, 1, 65, 8, 1, 4, 0) == -3               # TC_ESHAPE
    assert _raw(qkv, out, None, None, 1, 65, 8, 1, 0, 1) == -3
    assert _raw(qkv, out, big, big, 1, 64, 8, 1, 0, 0) == -3
    assert _raw(qkv, out, big, big, 1, 64, 8, 1, 65, 0) == -3
    assert _raw(qkv, out, rk, None, 1, 64, 8, 1, 4, 0) == -1             # TC_EINVAL: exactly one table
    assert _raw(qkv, out, None, rv, 1, 64, 8, 1, 4, 0) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    with pytest.raises(_lib.TooncrafterHipError, match="TC_ESHAPE"):
        hip.attention_temporal_rel(qkv, rk, rv, b=1, t=65, hw=8, heads=1, max_rel=4, causal=0)
    with pytest.raises(ValueError):
        hip.attention_temporal_rel(qkv[:64 * 8], rk, rv, b=1, t=64, hw=8, heads=1, max_rel=5, causal=0)   # table shape
    assert _raw(qkv, out, rk, rv, 1, 64, 8, 1, 4, 1) == 0                # the last accepted length


def test_torch_ops_bit_equal_to_ctypes(hip):
    from tooncrafter_amd.torch_ops import TorchLibOps
    t_ops = TorchLibOps()
    qkv = rnd(2 * 24 * 40, 3 * 320, seed=11)
    rk, rv = tables(16, seed=5)
    kw = dict(b=2, t=24, hw=40, heads=5, max_rel=16, causal=1)
    assert torch.equal(hip.attention_temporal_rel(qkv, rk, rv, **kw), t_ops.attention_temporal_rel(qkv, rk, rv, **kw))
    kw["max_rel"] = 0
    assert torch.equal(hip.attention_temporal_rel(qkv, None, None, **kw), t_ops.attention_temporal_rel(qkv, None, None, **kw))


# ------------------------------------------------------------------------------------------------ tiny UNet
# sha256 of the flagless tiny UNet's output on the fixture's 4-frame inputs (fp32 bytes), taken on the HIP backend on the commit
# before tc_attn_temporal_rel existed: models without the two flags compute what they computed
FLAGLESS_SHA = "04dde66766ea805d0e9255697636e3ce5491e5f6ef8010bfd42e3b4ff8010b74"


@pytest.fixture(scope="module")
def flagless_outputs(hip, golden):
    un = rc.tiny_unet().to(DEV)
    out = {}
    with torch.no_grad():
        for t in (4, 6):
            args, kw = rc.unet_inputs(golden, t, DEV)
            out[t] = _with_backend(hip, lambda: un(*args, **kw)).clone()
    return out


def test_flagless_unet_is_bit_equal_to_the_commit_before(flagless_outputs, golden):
    y = flagless_outputs[4].float().cpu().contiguous()
    assert rel_l2(y, torch.from_numpy(golden["y_plain4"])) < rc.UNET_BORROWED
    assert hashlib.sha256(y.numpy().tobytes()).hexdigest() == FLAGLESS_SHA


@pytest.mark.parametrize("variant", list(rc.VARIANTS))
def test_tiny_unet_vs_reference_golden(hip, golden, flagless_outputs, variant):
    un = rc.tiny_unet(variant)
    if rc.VARIANTS[variant][0]:
        rc.set_tables(un, golden)
    un = un.to(DEV)
    args, kw = rc.unet_inputs(golden, variant, DEV)
    with torch.no_grad():
        y = _with_backend(hip, lambda: un(*args, **kw)).clone()
    e = rel_l2(y.cpu(), torch.from_numpy(golden["y_" + variant]))
    d = rel_l2(y, flagless_outputs[rc.VARIANTS[variant][2]])
    bound = rc.unet_bound(variant)
    print(f"tiny UNet {variant} vs reference golden: {e:.3e} (bound {bound:.3e}); distance to the flagless model {d:.3e}")
    assert torch.isfinite(y).all()
    assert e < bound
    assert d > bound


def test_unet_hipgraph_replay_matches_eager(hip, golden):
    """One step of the "both" variant captured with torch.cuda.graph and replayed twice on refreshed inputs: the kernel
    allocates nothing and synchronises nothing, and the packed tables are fixed buffers."""
    un = rc.set_tables(rc.tiny_unet("both"), golden).to(DEV)
    (x, ts), kw = rc.unet_inputs(golden, "both", DEV)
    news = [(rnd(*x.shape, seed=21, dtype=torch.float32), torch.tensor([339], device=DEV)),
            (rnd(*x.shape, seed=22, dtype=torch.float32), torch.tensor([77], device=DEV))]

    def run():
        with torch.no_grad():
            eager = [un(xn, tn, **kw).clone() for xn, tn in news]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                un(x, ts, **kw)
            torch.cuda.current_stream().wait_stream(s)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                y = un(x, ts, **kw)
            replays = []
            for xn, tn in news:
                x.copy_(xn)
                ts.copy_(tn)
                gr.replay()
                torch.cuda.synchronize()
                replays.append(y.clone())
            return eager, replays
    eager, replays = _with_backend(hip, run)
    assert not torch.equal(eager[0], eager[1])
    assert torch.equal(eager[0], replays[0]) and torch.equal(eager[1], replays[1])
