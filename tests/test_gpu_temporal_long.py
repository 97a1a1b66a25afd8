"""tc_attn_temporal at 17 .. 64 frames (csrc/attention_temporal_long.hip): the long clips of the reference's --video_length N.

Against the PyTorch statement of the contract (tests/emu_ops.py: fp32 softmax) at the operator bound of
test_gpu_ops.py::test_attention_temporal (rel-L2 <= 8e-3; the kernel rounds its softmax weights to bf16 as
csrc/qkv_attn.hip does); exact data that catches a permuted key order or a row / column swap; no leak across clips
or from padded frames; t = 65 refused without a launch; the torch.ops binding bit-equal to ctypes; guard pages behind
every operand.
"""
import ctypes as C

import pytest
import torch

from emu_ops import EmuOps
from tooncrafter_amd import _lib

pytestmark = pytest.mark.gpu
DEV, BF16 = "cuda", torch.bfloat16
GRAN = 2 << 20


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def emu():
    return EmuOps()


def rnd(*shape, seed=0, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def rel_err(out, ref):
    o, r = out.double(), ref.double()
    return float((o - r).norm() / (r.norm() + 1e-30))


def _raw(lib, qkv, out, b, t, hw, heads, scale=0.125):
    return lib.tc_attn_temporal(qkv.data_ptr(), out.data_ptr(), b, t, hw, heads, scale, None)


# every t of the issue, each hw and each head count at least twice, both batch sizes; the last rows are the largest
# problems (level-0 widths, 64 frames, two clips)
_TS = [17, 24, 31, 32, 33, 48, 63, 64]
_CASES = [(t, hw, [1, 5, 10, 20][(i + j) % 4], 1 + (i + j) % 2) for i, t in enumerate(_TS) for j, hw in enumerate([7, 40, 640])]
_CASES += [(64, 640, 20, 2), (33, 640, 10, 2), (24, 40, 20, 2)]


@pytest.mark.parametrize("t,hw,heads,b", _CASES)
def test_long_temporal_vs_contract(hip, emu, t, hw, heads, b):
    qkv = rnd(b * t * hw, 3 * heads * 64, seed=t * 1000 + hw + heads)
    o = hip.attention_temporal(qkv, b=b, t=t, hw=hw, heads=heads)
    r = emu.attention_temporal(qkv, b=b, t=t, hw=hw, heads=heads)
    assert o.shape == r.shape and torch.isfinite(o).all()
    e = rel_err(o, r)
    print(f"temporal attn b{b} t{t} hw{hw} h{heads}: rel-L2 {e:.3e}")
    assert e <= 8e-3


@pytest.mark.parametrize("t", [24, 64])
def test_one_hot_keys_select_exact_rows(hip, t):
    """K of frame j = 64 e_j, Q of frame f = 64 e_sigma(f) with sigma(f) = (5 f + 3) mod t (asymmetric): the score of the
    selected key exceeds every other by 4096 * 0.125 = 512, so the softmax is exactly one-hot in fp32 and bf16, and the
    output row of frame f must equal V[sigma(f)] bit for bit.  A permuted k order in P^T . V^T or a swapped lane / register
    reading would pick another row."""
    b, hw, heads = 1, 3, 2
    c = heads * 64
    qkv = torch.zeros(b * t * hw, 3 * c)
    sigma = [(5 * f + 3) % t for f in range(t)]
    assert sorted(sigma) == list(range(t))
    for f in range(t):
        for p in range(hw):
            row = f * hw + p
            for h in range(heads):
                qkv[row, h * 64 + sigma[f]] = 64.0
                qkv[row, c + h * 64 + f] = 64.0
    v = torch.randn(t * hw, c, generator=torch.Generator().manual_seed(5)).to(BF16)
    qkv = qkv.to(BF16)
    qkv[:, 2 * c:] = v
    o = hip.attention_temporal(qkv.to(DEV), b=b, t=t, hw=hw, heads=heads, scale=0.125).cpu()
    want = torch.empty_like(v)
    for f in range(t):
        want[f * hw:(f + 1) * hw] = v[sigma[f] * hw:(sigma[f] + 1) * hw]
    assert torch.equal(o, want), f"{int((o != want).sum())} of {o.numel()} outputs differ"


@pytest.mark.parametrize("t", [17, 33, 40])
def test_clip_boundaries_and_padded_frames(hip, t):
    """b = 2 with huge values in every frame of clip 1: clip 0's output must not move (bit for bit against clip 0 alone).
    A padded key (t .. TT-1) read from the rows that follow -- clip 1's frames -- or a padded query row stored over them
    would show."""
    hw, heads = 40, 5
    c = heads * 64
    x0 = rnd(t * hw, 3 * c, seed=70 + t)
    x1 = rnd(t * hw, 3 * c, seed=90 + t, scale=3000.0)
    both = hip.attention_temporal(torch.cat([x0, x1]), b=2, t=t, hw=hw, heads=heads)
    alone = hip.attention_temporal(x0, b=1, t=t, hw=hw, heads=heads)
    assert torch.equal(both[:t * hw], alone)
    assert torch.isfinite(both).all()


def test_65_frames_refused_without_launch(hip):
    lib = _lib.load()
    assert _lib.TC_TEMPORAL_MAX_FRAMES == 64
    qkv = rnd(65 * 8, 3 * 64, seed=3)
    out = torch.full((65 * 8, 64), 7.0, dtype=BF16, device=DEV)
    assert _raw(lib, qkv, out, 1, 65, 8, 1) == -3                 # TC_ESHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    with pytest.raises(_lib.TooncrafterHipError, match="TC_ESHAPE"):
        hip.attention_temporal(qkv, b=1, t=65, hw=8, heads=1)
    assert _raw(lib, qkv[:64 * 8], out[:64 * 8], 1, 64, 8, 1) == 0      # the last accepted length


def test_torch_ops_bit_equal_to_ctypes_at_32_frames(hip):
    from tooncrafter_amd.torch_ops import TorchLibOps
    t_ops = TorchLibOps()
    qkv = rnd(2 * 32 * 40, 3 * 640, seed=11)
    a = hip.attention_temporal(qkv, b=2, t=32, hw=40, heads=10)
    b = t_ops.attention_temporal(qkv, b=2, t=32, hw=40, heads=10)
    assert torch.equal(a, b)
    m = torch.ops.tooncrafter.attention_temporal(qkv.to("meta"), 2, 32, 40, 10, 0.125)
    assert m.shape == a.shape


class _Region:
    """One hipMalloc of k * 2 MiB whose last `nbytes` bytes back a tensor (tests/test_gpu_guard.py's allocation, restated)."""
    _hip = None

    def __init__(self, nbytes, shape):
        if _Region._hip is None:
            _Region._hip = C.CDLL("libamdhip64.so")
            _Region._hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            _Region._hip.hipFree.argtypes = [C.c_void_p]
        hip = _Region._hip
        size = (nbytes + GRAN - 1) // GRAN * GRAN
        base, hole = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(base), size) == 0
        if hip.hipMalloc(C.byref(hole), GRAN) == 0:               # own, then release, the VA right behind the region
            hip.hipFree(hole)
        self.base, self.size = base.value, size
        self.ptr = base.value + size - nbytes
        assert self.ptr % 16 == 0
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<i2", "data": (self.ptr, False),
                                         "version": 2, "strides": None}

    def __del__(self):
        try:
            torch.cuda.synchronize()
            _Region._hip.hipFree(C.c_void_p(self.base))
        except Exception:
            pass


def guard(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    nbytes = t.numel() * t.element_size()
    assert t.dtype == BF16 and nbytes % 16 == 0
    reg = _Region(nbytes, t.shape)
    g = torch.as_tensor(reg, device=DEV).view(BF16)
    g._guard_region = reg
    g.copy_(t.to(DEV))
    assert g.data_ptr() == reg.ptr and g.data_ptr() + nbytes == reg.base + reg.size
    return g


@pytest.mark.parametrize("b,t,hw,heads", [(1, 24, 7, 1), (2, 24, 5, 3), (1, 64, 7, 1), (2, 64, 3, 2), (1, 33, 1, 1)])
def test_guard_pages(emu, b, t, hw, heads):
    """qkv and out each end at an unmapped page: the last pixel / head of the last clip reads and writes the final bytes."""
    lib = _lib.load()
    c = heads * 64
    qkv = guard(rnd(b * t * hw, 3 * c, seed=50 + t))
    out = guard(torch.zeros(b * t * hw, c, dtype=BF16))
    assert _raw(lib, qkv, out, b, t, hw, heads) == 0
    torch.cuda.synchronize()
    e = rel_err(out, emu.attention_temporal(qkv, b=b, t=t, hw=hw, heads=heads, scale=0.125))
    print(f"guard temporal attn b{b} t{t} hw{hw} h{heads}: rel-L2 {e:.3e}")
    assert e <= 8e-3
