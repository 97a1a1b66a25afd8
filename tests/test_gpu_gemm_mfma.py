"""The two MFMA shapes of the tiled GEMM K loops (csrc/gemm.hip gemm_kernel, csrc/gemm8.hip gemm8_kernel; TC_GEMM_MFMA =
16 | 32: v_mfma_f32_16x16x32_bf16 | v_mfma_f32_32x32x16_bf16 at the same wave tile, LDS image and fragment bytes).

Every test runs under BOTH arms of the switch, whatever the default is.  What can go wrong in arm 16 is a layout: the
fragment read (row lane & 15, chunk 4 ks + (lane >> 4) under the image's swizzle) and the accumulator -> LDS transposition
(column lane & 15, rows 4 (lane >> 4) + r), per tile size and per instance; so the cases are
  * a transpose-detecting product on every instance (four tile sizes x both K loops, and the 8-wave kernel);
  * ragged M / N / K, one K-step, every gather, split-K, GEGLU and bias + residual against the fp32 statement of the operator
    (tests/emu_ops.py) at the suite's tolerance (test_gpu_ops.check), and arm against arm within 2^-6 max(|out|, 1): the same
    fp32 products in another summation order (the bound of test_gpu_conv_halo.py);
  * the integer cases of tests/gemm_exact_cases.py that target gemm_kernel<...> and gemm8_kernel<...>, to the bit;
  * 8-wave == 4-wave bit for bit (the two files must sit on the same shape and the same order at the same time);
  * ten identical launches (race screen)."""
import pytest
import torch

import gemm_exact_cases as X
from emu_ops import EmuOps
from test_gpu_gemm_exact import launch
from test_gpu_ops import check, rnd
from tooncrafter_amd._lib import ACT_GEGLU

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
ARMS = (16, 32)
env = X.env

# the instances, forced by their switches: the four 4-wave tiles with the plain and the pipelined K loop, and the 8-wave kernel
TILES = [dict(TC_GEMM_TILE=t, TC_GEMM_PIPE=p) for t in ("22", "21", "12", "11") for p in (0, 1)]
EIGHT = dict(TC_GEMM8=2)


def _id(e):
    return "-".join(f"{k[3:].lower()}{v}" for k, v in e.items())


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def emu():
    return EmuOps(round_bf16=True)


def _arms(route, fn):
    """fn() under the forced route with TC_GEMM_MFMA = 16 and = 32 -> {arm: output}"""
    out = {}
    for arm in ARMS:
        with env(TC_GEMM_MFMA=arm, **route):
            out[arm] = fn()
    torch.cuda.synchronize()
    return out


def _same_products(out, what):
    d = (out[16].float() - out[32].float()).abs().max().item()
    bound = 2.0 ** -6 * max(out[32].float().abs().max().item(), 1.0)
    print(f"{what}: arm 16 vs arm 32 max-abs {d:.3e} (bound {bound:.3e})")
    assert d <= bound, f"{what}: the arms differ by {d}: more than another summation order of the same products"


# ---------------------------------------------------------------------------------------------- transpose-detecting
@pytest.mark.parametrize("route", TILES + [EIGHT], ids=_id)
@pytest.mark.parametrize("arm", ARMS)
def test_transpose_detecting(hip, route, arm):
    """Identity-like A against an asymmetric W (test_gpu_gemm8.py): a swapped fragment / C-write mapping cannot pass."""
    m = n = k = 512 if route is EIGHT else 192
    a = torch.eye(m, k, device=DEV, dtype=BF16)
    w = ((torch.arange(n, device=DEV)[:, None] * 3 + torch.arange(k, device=DEV)[None, :] % 7).float())
    w = (w / w.max()).to(BF16)
    with env(TC_GEMM_MFMA=arm, **route):
        out = hip.gemm(a, w)
    assert torch.equal(out, w.t().contiguous()), f"arm {arm} {route}: fragment or C-write layout is wrong"


# ---------------------------------------------------------------------------------------------- ragged shapes
def _lin(m, n, k, res=False):
    a, w, bias = rnd(m, k, seed=m + k), rnd(n, k, seed=n + 2, scale=k ** -0.5), rnd(n, seed=3, dtype=torch.float32)
    return a, w, bias, dict(residual=rnd(m, n, seed=4) if res else None)


def _conv3x3():
    frames, h, w_, cin, n = 2, 10, 16, 64, 136
    conv = dict(kind="3x3", frames=frames, cin=cin, h_in=h, w_in=w_, h_out=h, w_out=w_, stride=1, upsample=False)
    m = frames * h * w_
    return (rnd(m, cin, seed=21), rnd(n, 9 * cin, seed=22, scale=(9 * cin) ** -0.5), rnd(n, seed=23, dtype=torch.float32),
            dict(conv=conv, residual=rnd(m, n, seed=25)))


def _conv_t3():
    frames, hw, cin, n = 32, 7, 64, 136
    conv = dict(kind="t3", frames=frames, t_len=16, cin=cin, h_out=1, w_out=hw)
    m = frames * hw
    return (rnd(m, cin, seed=31), rnd(n, 3 * cin, seed=32, scale=(3 * cin) ** -0.5), rnd(n, seed=33, dtype=torch.float32),
            dict(conv=conv, residual=rnd(m, n, seed=34)))


def _geglu():
    from tooncrafter_amd.lvdm.common import pack_geglu
    m, n, k = 267, 256, 320
    w, bias = pack_geglu(rnd(n, k, seed=12, scale=k ** -0.5, dtype=torch.float32), rnd(n, seed=13, dtype=torch.float32))
    return rnd(m, k, seed=11), w, bias, dict(act=ACT_GEGLU)


T22, T11 = dict(TC_GEMM_TILE="22"), dict(TC_GEMM_TILE="11")
# (name, operands, routes).  K = 64 is one K-step: the 8-wave kernel needs two and is not asked.  Split-K is a decision of
# the default route of that shape (tests/gemm_exact_cases.py tile-lin-splitk2): a forced tile would switch it off
RAGGED = [
    ("m267-n136-k192", lambda: _lin(267, 136, 192), (T22, T11, dict(TC_GEMM_TILE="21"), dict(TC_GEMM_TILE="12"), EIGHT)),
    ("k200-ragged-last-step", lambda: _lin(267, 136, 200), (T22, T11, EIGHT)),
    ("k64-one-step", lambda: _lin(267, 136, 64), (T22, T11)),
    ("bias-residual", lambda: _lin(267, 136, 192, res=True), (T22, T11, EIGHT)),
    ("conv3x3", _conv3x3, (T22, T11, EIGHT)),
    ("conv-t3", _conv_t3, (T22, T11, EIGHT)),
    ("splitk2-k1088", lambda: _lin(267, 136, 1088, res=True), (dict(TC_GEMM_SPLITK=2),)),
    ("geglu-n256-k320", _geglu, (T22, dict(TC_GEMM_TILE="12"), EIGHT)),
]


@pytest.mark.parametrize("name,make,routes", RAGGED, ids=[r[0] for r in RAGGED])
def test_ragged_against_emulation(hip, emu, name, make, routes):
    a, w, bias, kw = make()
    ref = emu.gemm(a, w, bias, **kw)
    for route in routes:
        out = _arms(route, lambda: hip.gemm(a, w, bias, **kw))
        for arm in ARMS:
            check(out[arm], ref, f"{name} {_id(route)} arm {arm}")
        _same_products(out, f"{name} {_id(route)}")


# ---------------------------------------------------------------------------------------------- the integer cases
EXACT = [c for c in X.CASES if c.target.startswith(("gemm_kernel<", "gemm8_kernel<"))]


@pytest.fixture(scope="module")
def expected():
    """name -> (inputs, stored reference): computed once, on the CPU, shared by the arms, never modified"""
    cache = {}

    def get(c):
        if c.name not in cache:
            inp = X.inputs(c)
            cache[c.name] = (inp, X.store(c, X.reference(c, inp)))
        return cache[c.name]
    return get


@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
@pytest.mark.parametrize("arm", ARMS)
def test_exact(hip, expected, c, arm):
    inp, want = expected(c)
    with env(TC_GEMM_MFMA=arm):
        out, _ = launch(hip, c, inp)
    report = X.differences(c, out.cpu(), want)
    assert report is None, f"arm {arm}: {report}"


# ---------------------------------------------------------------------------------------------- 8-wave == 4-wave
@pytest.mark.parametrize("m,n,k", [(300, 256, 192), (1000, 520, 392)])
@pytest.mark.parametrize("arm", ARMS)
def test_eight_wave_equals_four_wave(hip, emu, m, n, k, arm):
    a, w, bias, kw = _lin(m, n, k, res=True)
    got = {}
    for name, route in (("8-wave", dict(TC_GEMM8=2, TC_GEMM_SPLITK=0)), ("128x128", dict(TC_GEMM_TILE="22")), ("64x64", dict(TC_GEMM_TILE="11"))):
        with env(TC_GEMM_MFMA=arm, **route):
            got[name] = hip.gemm(a, w, bias, **kw)
    torch.cuda.synchronize()
    check(got["8-wave"], emu.gemm(a, w, bias, **kw), f"8-wave {m}x{n}x{k} arm {arm}")
    assert torch.equal(got["8-wave"], got["128x128"]), f"arm {arm}: 8-wave and 128x128 kernels differ bit-wise"
    assert torch.equal(got["8-wave"], got["64x64"]), f"arm {arm}: 8-wave and 64x64 kernels differ bit-wise"


# ---------------------------------------------------------------------------------------------- race screen
@pytest.mark.parametrize("route", [T22, EIGHT], ids=_id)
@pytest.mark.parametrize("arm", ARMS)
def test_repeated_launches_are_bit_identical(hip, route, arm):
    m, n, k = 2048, 640, 640
    a, w, res = rnd(m, k, seed=51), rnd(n, k, seed=52, scale=k ** -0.5), rnd(m, n, seed=53)
    with env(TC_GEMM_MFMA=arm, **route):
        first = hip.gemm(a, w, residual=res)
        for _ in range(10):
            assert torch.equal(hip.gemm(a, w, residual=res), first), f"arm {arm}: a launch differs: a fragment was read before it landed"


# ---------------------------------------------------------------------------------------------- the qkv projection (TC_QKV_MFMA)
def _qkv_fp64(x, raw, bq, b, t, hw, heads):
    """softmax(q k^T / 8) v over the frames of every pixel, q / k / v = Linear(x), heads re-concatenated, in fp64
    (test_gpu_qkv_attn.py's statement, with the bias)"""
    c = heads * 64
    qkv = x.double().cpu() @ raw.double().cpu().t()
    if bq is not None:
        qkv = qkv + bq.double().cpu()[None, :]
    q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(b, t, hw, heads, 64).permute(0, 2, 3, 1, 4) for i in range(3))
    o = ((q @ k.transpose(-1, -2)) * 64 ** -0.5).softmax(-1) @ v
    return o.permute(0, 3, 1, 2, 4).reshape(b * t * hw, c)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("t,heads", [(16, 1), (16, 5)], ids=["t16-h1", "t16-h5"])
def test_qkv_projection_arms(hip, t, heads, bias):
    """tc_temporal_qkv_attn (csrc/qkv_attn_tile.h qa_project) under TC_QKV_MFMA = 16 and 32 at the smallest shapes of
    test_gpu_qkv_attn.py (one tile of 8 pixels; one head and five; the long-clip kernel of qkv_attn_long.hip is not behind
    the switch): each arm against that file's fp64 statement -- its inputs (test_fused_vs_fp64_reference_attention: x from
    seed 21, weights from seed 5) and its tolerance, 6e-3 --, arm against arm within the bound of another summation order,
    repeated launches identical.

    What the tolerance leaves.  The statement takes the UNROUNDED fp32 weights, the operator their bf16 packing, and rounds
    q / k / v, the softmax weights and the output to bf16: on the CPU emulation of exactly those roundings (tests/emu_ops.py,
    no kernel involved) the figure is 5.4e-3 at every width, and over ten seeds it spreads 4.6 .. 6.8e-3 at one head and 8
    pixels (8 softmaxes of 16 x 16 carry the whole norm) against 5.2 .. 5.6e-3 at 48 pixels.  A first version of this test
    drew x and the weights from seeds 11 / 1 (the inputs of that file's OTHER test, which has another reference): there one
    head gives 6.853e-03 on both arms, bit-identical, and the emulation 6.80e-3 on the same inputs -- the sample, not the
    kernel; five heads gave 5.605e-03.  The inputs are now the ones of the statement the tolerance was set for."""
    from test_gpu_qkv_attn import _w, _x
    assert t == 16
    b, hw, c = 1, 8, heads * 64
    x = _x(b, hw, c, seed=21)
    raw, w = _w(c, seed=5)
    bq = rnd(3 * c, seed=9, scale=0.2, dtype=torch.float32) if bias else None
    ref = _qkv_fp64(x, raw, bq, b, t, hw, heads)
    out = {}
    for arm in ARMS:
        with env(TC_QKV_MFMA=arm, TC_QKV_ATTN=2):
            assert hip.temporal_qkv_attn_eligible(b=b, t=t, hw=hw, c=c, heads=heads, ldx=x.stride(0))
            out[arm] = hip.temporal_qkv_attn(x, w, bq, b=b, t=t, hw=hw, heads=heads)
            for _ in range(3):
                assert torch.equal(hip.temporal_qkv_attn(x, w, bq, b=b, t=t, hw=hw, heads=heads), out[arm]), f"arm {arm}: repeated launch differs"
        torch.cuda.synchronize()
    errs = {arm: float((out[arm].double().cpu() - ref).norm() / ref.norm()) for arm in ARMS}
    for arm in ARMS:                                 # every figure is printed before any is judged
        print(f"qkv + attention t={t} heads={heads} bias={bias} arm {arm} vs fp64: rel-L2 {errs[arm]:.3e}")
    _same_products(out, f"qkv + attention t={t} heads={heads} bias={bias}")
    for arm in ARMS:
        assert errs[arm] < 6e-3, f"arm {arm}: rel-L2 {errs[arm]:.3e}"
