"""The temporal q / k / v projection and its attention over 17 .. 64 frames as ONE launch (tc_temporal_qkv_attn beyond 16
frames: csrc/qkv_attn_long.hip, frame count padded to TT = 32 | 64 slots, 128 / TT pixels per block; reference
lvdm/modules/attention.py:96-134 over the frames of a pixel at a --video_length above 16).

Every test runs with TC_QKV_ATTN=2 (every shape the kernel can take), whatever the default rule admits.  Checked against
(a) the two launches it replaces -- tc_gemm_bf16 + tc_attn_temporal (csrc/attention_temporal_long.hip), which round alike;
(b) the emulated operator; (c) the fp64 statement of the reference's attention, bounded by the emulated contract's own
error; (d) exact data: selector weights and one-hot softmaxes, where the output is a known permutation of the input bit
for bit.  Padded frame slots and clip boundaries are probed with poisoned neighbours inside one larger allocation (NaN rows
around x, canaries around out): a mistake shows as a wrong number.
"""
import pytest
import torch

from conftest import TINY_UNET_CFG, rel_l2, sub_state_dict
from emu_ops import EmuOps
from test_gpu_ops import check, rnd
from test_qkv_attn_long_cpu import exact_case
from tooncrafter_amd import ops, synth
from tooncrafter_amd.lvdm.common import pack_linear

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(autouse=True)
def _every_shape(monkeypatch):
    monkeypatch.setenv("TC_QKV_ATTN", "2")


def _w(c, seed=1):
    raw = torch.cat([rnd(c, c, seed=seed + i, scale=1.4 * c ** -0.5, dtype=torch.float32) for i in range(3)], 0)
    return raw, pack_linear(raw)


def _x(b, t, hw, c, seed=11, pitch=None):
    full = rnd(b * t * hw, pitch or c, seed=seed, scale=1.2) + 0.1
    return full.to(BF16)[:, :c]


# t, b, hw, c, pitch
CASES = [(17, 1, 4, 64, None), (24, 2, 40, 640, None), (31, 1, 12, 320, None), (32, 2, 160, 1280, None), (32, 3, 52, 640, None),
         (32, 1, 24, 320, None), (33, 1, 6, 320, None), (48, 2, 40, 1280, None), (64, 1, 2, 64, None), (64, 1, 64, 640, 1920),
         (64, 2, 40, 1280, None), (64, 2, 640, 640, None)]


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("t,b,hw,c,pitch", CASES, ids=[f"t{c[0]}-b{c[1]}-hw{c[2]}-c{c[3]}" for c in CASES])
def test_fused_vs_two_launches_and_emulation(hip, t, b, hw, c, pitch, bias):
    heads = c // 64
    tag = f"t = {t}, b = {b}, hw = {hw}, C = {c}"
    x = _x(b, t, hw, c, pitch=pitch)
    raw, w = _w(c)
    bq = rnd(3 * c, seed=9, scale=0.2, dtype=torch.float32) if bias else None
    assert hip.temporal_qkv_attn_eligible(b=b, t=t, hw=hw, c=c, heads=heads, ldx=x.stride(0))
    kw = dict(b=b, t=t, hw=hw, heads=heads)
    out = hip.temporal_qkv_attn(x, w, bq, **kw)
    torch.cuda.synchronize()
    ref = hip.attention_temporal(hip.gemm(x.contiguous(), w, bq), **kw)
    check(out, ref, f"{tag}: fused vs gemm + attention_temporal", rel=3e-3)
    if b * t * hw * c <= 8192 * 640:
        emu = EmuOps(round_bf16=True, tqa=True)
        want = emu.temporal_qkv_attn(x.cpu(), w.cpu(), None if bq is None else bq.cpu(), **kw)
        e = rel_l2(out.cpu(), want)
        print(f"{tag}: fused vs emulation rel-L2 {e:.3e}")
        assert e <= 8e-3
    again = hip.temporal_qkv_attn(x, w, bq, **kw)
    assert torch.equal(out, again), "repeated launch differs"


@pytest.mark.parametrize("t", [24, 64])
def test_fused_vs_fp64_reference_attention(hip, t):
    """softmax(q k^T / 8) v over the frames of every pixel, q / k / v = Linear(x), heads re-concatenated, in fp64.  The
    bound is the emulated contract's own error against the same fp64 result (bf16 q / k / v and output, fp32 softmax
    weights) plus 25 %: the kernel also rounds its softmax weights to bf16, about 1e-3 added in quadrature to ~6e-3, i.e.
    ~2 %, and sums in another order."""
    b, hw, c = 1, 48, 640
    heads = c // 64
    x = _x(b, t, hw, c, seed=21)
    raw, w = _w(c, seed=5)
    kw = dict(b=b, t=t, hw=hw, heads=heads)
    out = hip.temporal_qkv_attn(x, w, None, **kw).double().cpu()
    qkv = x.double().cpu() @ raw.double().cpu().t()
    q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(b, t, hw, heads, 64).permute(0, 2, 3, 1, 4) for i in range(3))
    o = ((q @ k.transpose(-1, -2)) * 64 ** -0.5).softmax(-1) @ v                       # [b, hw, heads, t, 64]
    ref = o.permute(0, 3, 1, 2, 4).reshape(b * t * hw, c)
    emu = EmuOps(round_bf16=True, tqa=True).temporal_qkv_attn(x.cpu(), w.cpu(), None, **kw).double()
    err = float((out - ref).norm() / ref.norm())
    e_emu = float((emu - ref).norm() / ref.norm())
    print(f"t = {t}: fused qkv + temporal attention vs fp64 reference: rel-L2 {err:.3e}; emulated contract {e_emu:.3e}")
    assert err <= 1.25 * e_emu


@pytest.mark.parametrize("t", [24, 64])
def test_exact_data_through_the_projection(hip, t):
    x, w, want = exact_case(t)
    out = hip.temporal_qkv_attn(x.to(DEV), w.to(DEV), None, b=1, t=t, hw=4, heads=3).cpu()
    bad = (out.view(torch.int16) != want.view(torch.int16)).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"rows (frame * 4 + pixel) that are not the payload of frame sigma(f): {bad[:16]}"


@pytest.mark.parametrize("t", [24, 48])
def test_attention_is_over_frames_of_the_same_pixel(hip, t):
    """Changing ONE row changes the t output rows of its pixel in its clip and nothing else."""
    b, hw, c = 2, 40, 640
    x = _x(b, t, hw, c, seed=31).contiguous()
    _, w = _w(c, seed=7)
    kw = dict(b=b, t=t, hw=hw, heads=c // 64)
    y0 = hip.temporal_qkv_attn(x, w, None, **kw)
    x2 = x.clone()
    pix, bb = 13, 1
    rows = (bb * t + torch.arange(t, device=x.device)) * hw + pix
    x2[rows[5]] = (x2[rows[5]].float() * -0.7 + 0.2).to(BF16)                         # frame 5 of pixel 13 of clip 1
    y1 = hip.temporal_qkv_attn(x2, w, None, **kw)
    changed = (y0 != y1).any(dim=1).nonzero().flatten().tolist()
    assert set(changed) == set(rows.tolist()), changed            # every query of the pixel attends to the changed key
    cols = (y0[rows] != y1[rows]).any(dim=0)
    assert int(cols.sum()) > c // 2                                                     # every head's slice moved


@pytest.mark.parametrize("t", [17, 33, 40])
def test_clip_boundaries_and_padded_slots(hip, t):
    """The padded frame slots of clip 0 would, read unmasked, be rows of clip 1 (scaled by 3000 here) or rows behind the
    tensor (NaN here); a row stored for a padded slot would land in clip 1 or behind `out` (canaries here)."""
    b, hw, c = 2, 40, 320
    heads = c // 64
    rows = t * hw
    x = _x(b, t, hw, c, seed=51).contiguous()
    x[rows:] = (x[rows:].float() * 3000).to(BF16)
    _, w = _w(c, seed=13)
    out = hip.temporal_qkv_attn(x, w, None, b=b, t=t, hw=hw, heads=heads)
    alone = hip.temporal_qkv_attn(x[:rows].clone(), w, None, b=1, t=t, hw=hw, heads=heads)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out[:rows], alone), "clip 0 depends on clip 1"
    pad = ((32 if t <= 32 else 64) - t + 1) * hw          # every row a padded slot of the last clip could name is allocated
    x_big = torch.full((b * rows + 2 * pad, c + 64), float("nan"), dtype=BF16, device=DEV)
    x_big[pad:pad + b * rows, :c] = x
    out_big = torch.full((b * rows + 2 * pad, c + 64), 7.0, dtype=BF16, device=DEV)
    got = hip.temporal_qkv_attn(x_big[pad:pad + b * rows, :c], w, None, b=b, t=t, hw=hw, heads=heads,
                                out=out_big[pad:pad + b * rows, :c])
    torch.cuda.synchronize()
    assert torch.equal(got, out), "interior slices give other bits than the plain call"
    assert torch.equal(out_big[pad:pad + b * rows, :c], out)
    assert bool((out_big[:pad] == 7.0).all()) and bool((out_big[pad + b * rows:] == 7.0).all()), "a row in front of / behind out was written"
    assert bool((out_big[:, c:] == 7.0).all()), "columns beside out were written"


def test_refusals_launch_nothing(hip, monkeypatch):
    from tooncrafter_amd._lib import TooncrafterHipError
    c, heads = 640, 10
    _, w = _w(c)
    x = _x(1, 65, 8, c)
    out = torch.full((65 * 8, c), 7.0, dtype=BF16, device=DEV)
    assert not hip.temporal_qkv_attn_eligible(b=1, t=65, hw=8, c=c, heads=heads)
    with pytest.raises(TooncrafterHipError, match="TC_ESHAPE"):
        hip.temporal_qkv_attn(x, w, None, b=1, t=65, hw=8, heads=heads, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert not hip.temporal_qkv_attn_eligible(b=1, t=32, hw=6, c=c, heads=heads)           # hw % 4
    assert hip.temporal_qkv_attn_eligible(b=1, t=32, hw=4, c=c, heads=heads)
    assert not hip.temporal_qkv_attn_eligible(b=1, t=64, hw=5, c=c, heads=heads)           # hw % 2
    out6 = torch.full((32 * 6, c), 7.0, dtype=BF16, device=DEV)
    with pytest.raises(TooncrafterHipError, match="TC_ESHAPE"):
        hip.temporal_qkv_attn(_x(1, 32, 6, c), w, None, b=1, t=32, hw=6, heads=heads, out=out6)
    torch.cuda.synchronize()
    assert bool((out6 == 7.0).all())
    assert not hip.temporal_qkv_attn_eligible(b=2, t=8, hw=640, c=c, heads=heads)           # below 16 frames: the two launches
    assert hip.temporal_qkv_attn_eligible(b=2, t=16, hw=640, c=c, heads=heads)              # 16 frames answer as before
    assert not hip.temporal_qkv_attn_eligible(b=2, t=16, hw=636, c=c, heads=heads)
    assert not hip.temporal_qkv_attn_eligible(b=2, t=32, hw=640, c=c, heads=8)              # c = heads * 64
    monkeypatch.setenv("TC_QKV_ATTN", "0")
    assert not hip.temporal_qkv_attn_eligible(b=2, t=32, hw=640, c=c, heads=heads)
    assert not hip.temporal_qkv_attn_eligible(b=2, t=16, hw=640, c=c, heads=heads)


def test_custom_op_binding_gives_the_same_bits(hip):
    from tooncrafter_amd import torch_ops
    tl = torch_ops.TorchLibOps()
    b, t, hw, c = 1, 32, 64, 640
    x, (_, w) = _x(b, t, hw, c, seed=41), _w(c, seed=3)
    bq = rnd(3 * c, seed=9, scale=0.2, dtype=torch.float32)
    kw = dict(b=b, t=t, hw=hw, heads=c // 64)
    assert torch.equal(tl.temporal_qkv_attn(x, w, None, **kw), hip.temporal_qkv_attn(x, w, None, **kw))
    assert torch.equal(tl.temporal_qkv_attn(x, w, bq, **kw), hip.temporal_qkv_attn(x, w, bq, **kw))
    bf = dict(dtype=BF16, device="meta")
    y = torch_ops.load().temporal_qkv_attn(torch.empty(b * t * hw, c, **bf), torch.empty(3 * c, c, **bf), None, b, t, hw, c // 64, 0.125)
    assert y.shape == (b * t * hw, c) and y.dtype == BF16 and y.device.type == "meta"


def test_block_routes_through_the_fused_operator(hip, monkeypatch):
    """A level-1 BasicTransformerBlock (temporal flavour) at 32 frames: mode 2 takes the one launch once per
    self-attention, mode 0 never."""
    from tooncrafter_amd.lvdm.attention import BasicTransformerBlock
    from tooncrafter_amd.lvdm.common import Act
    torch.manual_seed(0)
    blk = BasicTransformerBlock(640, 10, 64, context_dim=None).eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.normal_(0, 0.04)
        for i in (1, 2, 3):
            getattr(blk, f"norm{i}").weight.add_(1.0)
    blk = blk.cuda()
    prev = ops.set_backend(hip)
    try:
        b, t, h, w = 1, 32, 8, 16
        x = rnd(b * t * h * w, 640, seed=41)
        act = Act(x, b, t, h, w)
        calls = []
        real = hip.temporal_qkv_attn
        monkeypatch.setattr(hip, "temporal_qkv_attn", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        with torch.no_grad():
            y2 = blk.forward_temporal(x, act)
            n2 = len(calls)
            monkeypatch.setenv("TC_QKV_ATTN", "0")
            y0 = blk.forward_temporal(x, act)
        assert n2 == 2 and len(calls) == 2          # attn1 and attn2 (context = None: self attention again), once each
        check(y2, y0, "temporal block at 32 frames, qkv + attention as one launch on vs off", rel=8e-3)
    finally:
        ops.set_backend(prev)


# ------------------------------------------------------------------------------------------------ tiny UNet
def _tiny_unet(tiny_sd, t):
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    un = UNetModel(**dict(TINY_UNET_CFG, temporal_length=t)).eval()
    un.load_state_dict(sub_state_dict(tiny_sd, "model.diffusion_model."), strict=True)
    return un.to(DEV)


def _tiny_inputs(t, seed):
    inp = synth.synth_inputs(1, t, 8, 8, context_dim=TINY_UNET_CFG["context_dim"], n_img_tokens_per_frame=0, seed=seed)
    img = torch.randn(1, 256, TINY_UNET_CFG["context_dim"], generator=torch.Generator().manual_seed(seed + 1))
    inp["cond"] = torch.cat([inp["cond"], img], 1)
    return inp


def _with_backend(backend, fn):
    prev = ops.set_backend(backend)
    try:
        return fn()
    finally:
        ops.set_backend(prev)


@pytest.mark.parametrize("t", [24, 32])
def test_tiny_unet_vs_contract_and_oracle(hip, tiny_sd, monkeypatch, t):
    from oracle import unet as ounet
    un = _tiny_unet(tiny_sd, t)
    inp = _tiny_inputs(t, 40 + t)
    ts = torch.tensor([601])
    args = dict(context=inp["cond"].to(DEV), fs=inp["fs"].to(DEV), x_parts=[inp["x_T"].to(DEV), inp["c_concat"].to(DEV)])
    fused_hw, two_hw = [], []
    real_f, real_t = hip.temporal_qkv_attn, hip.attention_temporal
    monkeypatch.setattr(hip, "temporal_qkv_attn", lambda *a, **k: (fused_hw.append(k["hw"]), real_f(*a, **k))[1])
    monkeypatch.setattr(hip, "attention_temporal", lambda *a, **k: (two_hw.append(k["hw"]), real_t(*a, **k))[1])
    with torch.no_grad():
        y = _with_backend(hip, lambda: un(None, ts.to(DEV), **args)).cpu()
        n_fused, n_two = list(fused_hw), list(two_hw)
        monkeypatch.setenv("TC_QKV_ATTN", "0")
        fused_hw.clear(), two_hw.clear()
        un.reset_conditioning()
        _with_backend(hip, lambda: un(None, ts.to(DEV), **args))
        off_two = list(two_hw)
        assert not fused_hw
        un.reset_conditioning()
        y_emu = _with_backend(EmuOps(), lambda: un(None, ts.to(DEV), **args)).cpu()
        ref = ounet.unet_forward(sub_state_dict(tiny_sd, "model.diffusion_model."), dict(TINY_UNET_CFG, temporal_length=t),
                                 torch.cat([inp["x_T"], inp["c_concat"]], 1), ts, inp["cond"], inp["fs"])
    # with the switch off every temporal self-attention takes the two launches: that run lists them, per level
    assert {64, 16, 4, 1} == set(off_two), off_two
    for hw in (64, 16, 4):
        assert n_fused.count(hw) == off_two.count(hw) >= 1 and hw not in n_two, (hw, n_fused, n_two)
    assert n_two.count(1) == off_two.count(1) >= 1 and 1 not in n_fused              # hw = 1: no 128 / TT pixels to fill a tile
    e_emu, e_ref = rel_l2(y, y_emu), rel_l2(y, ref)
    print(f"tiny UNet T = {t}, one-launch qkv + attention: HIP vs emulated contract {e_emu:.3e}, vs fp32 oracle {e_ref:.3e}")
    assert y.shape == (1, 4, t, 8, 8) and torch.isfinite(y).all()
    assert e_emu <= 3e-2 and e_ref <= 3e-2


def test_tiny_unet_32_frames_hipgraph_replay_matches_eager(hip, tiny_sd):
    un = _tiny_unet(tiny_sd, 32)
    inp = _tiny_inputs(32, 77)
    ts = torch.tensor([339], device=DEV)
    args = dict(context=inp["cond"].to(DEV), fs=inp["fs"].to(DEV), x_parts=[inp["x_T"].to(DEV), inp["c_concat"].to(DEV)])

    def run():
        with torch.no_grad():
            eager = un(None, ts, **args).clone()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                un(None, ts, **args)
            torch.cuda.current_stream().wait_stream(s)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                y = un(None, ts, **args)
            gr.replay()
            torch.cuda.synchronize()
            return eager, y.clone()
    eager, replay = _with_backend(hip, run)
    assert torch.equal(eager, replay)
