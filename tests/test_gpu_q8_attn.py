"""The 8-bit spatial self-attention (csrc/attention_q8.hip, ABI 14) against its CPU restatement (tests/q8_attn_ref.py):
the K / V quantiser bit for bit, the attention to rel-L2 <= 2e-3 (only the fp32 summation order and v_exp_f32 differ; both
sides round the output to bf16), both bindings bit-identical, operands at an allocation's end, graph replay == eager."""
import ctypes as C

import pytest
import torch

import q8_attn_ref as R
from conftest import rel_l2
from test_gpu_guard import _Region
from tooncrafter_amd import _lib, ops
from tooncrafter_amd.ops import HipOps

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
TOL = 2e-3


@pytest.fixture(scope="module")
def hip():
    return HipOps()


def _qkv(batch, heads, lq, lk, mag=1.0, seed=0, fused=False):
    g = torch.Generator().manual_seed(seed)
    hd = heads * 64
    if fused:                                     # strided column slices of one [rows, 3C] qkv tensor (lq == lk)
        qkv = (torch.randn(batch * lq, 3 * hd, generator=g) * mag).to(BF16).to(DEV)
        return qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]
    q = (torch.randn(batch * lq, hd, generator=g) * mag).to(BF16).to(DEV)
    k = (torch.randn(batch * lk, hd, generator=g) * mag).to(BF16).to(DEV)
    v = torch.randn(batch * lk, hd, generator=g).to(BF16).to(DEV)
    return q, k, v


def _check(hip, q, k, v, batch, heads, lq, lk, scale=0.125):
    got = hip.attention_q8(q, k, v, batch=batch, heads=heads, lq=lq, lk=lk, scale=scale).float().cpu()
    ref = R.attention_rows(q.float().cpu(), k.float().cpu(), v.float().cpu(), batch=batch, heads=heads, lq=lq, lk=lk,
                           scale=scale).to(BF16).float()
    assert torch.isfinite(got).all()
    e = rel_l2(got, ref)
    exact = R.attention_rows(q.float().cpu(), k.float().cpu(), v.float().cpu(), batch=batch, heads=heads, lq=lq, lk=lk,
                             scale=scale, qk=None, pv_mx=False, dtype=torch.float64)
    print(f"q8 attention b{batch} h{heads} lq{lq} lk{lk}: rel-L2 vs restatement {e:.2e}, vs fp64 softmax {rel_l2(got, exact):.2e}")
    assert e <= TOL
    return got


def test_quant_kv_bytes_equal_restatement(hip):
    batch, heads, lk = 2, 3, 150                       # 3 tiles, the last with 22 keys: zero padding is part of the bytes
    _, k, v = _qkv(batch, heads, 1, lk, seed=3)
    k[5, 64:128] = 0                                   # an all-zero row: scale 1, bytes 0
    p = hip._q8_params(k[:batch], k, v, torch.empty(batch, heads * 64, dtype=BF16, device=DEV), batch, heads, 1, lk, 0.125)
    nbytes = hip.lib.tc_attn_q8_workspace(C.byref(p))
    nt = -(-lk // R.KT)
    assert nbytes == batch * heads * nt * R.REC
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
    _lib.check(hip.lib.tc_attn_q8_quant_kv(C.byref(p), 0), "tc_attn_q8_quant_kv")
    torch.cuda.synchronize()
    got = ws.cpu().view(batch, heads, nt, R.REC)
    kc, vc = k.float().cpu(), v.float().cpu()
    for b in range(batch):
        for h in range(heads):
            cs = slice(h * 64, h * 64 + 64)
            want = R.pack_records(kc[b * lk:(b + 1) * lk, cs], vc[b * lk:(b + 1) * lk, cs])
            assert torch.equal(got[b, h, :, :8576], want[:, :8576]), f"(b {b}, h {h}): quantised bytes differ"


@pytest.mark.parametrize("batch,heads,lq,lk", [(2, 5, 2560, 2560), (4, 10, 640, 640), (1, 2, 1000, 1000),
                                               (2, 3, 77, 77), (3, 1, 33, 33)])
def test_attention_q8_matches_restatement(hip, batch, heads, lq, lk):
    q, k, v = _qkv(batch, heads, lq, lk, seed=lq + lk)
    _check(hip, q, k, v, batch, heads, lq, lk)


def test_attention_q8_strided_qkv_slices(hip):
    q, k, v = _qkv(2, 5, 640, 640, seed=11, fused=True)
    _check(hip, q, k, v, 2, 5, 640, 640)


@pytest.mark.parametrize("mag", [1e-3, 30.0])
def test_attention_q8_magnitudes(hip, mag):
    q, k, v = _qkv(1, 2, 300, 300, mag=mag, seed=int(mag * 1000) % 97)
    _check(hip, q, k, v, 1, 2, 300, 300)


def test_attention_q8_dominant_and_equal_keys(hip):
    lq = lk = 200
    q, k, v = _qkv(1, 2, lq, lk, seed=5)
    k[:, :64] = k[:1, :64]                                       # head 0: every key equal -> mean of v
    k[77, 64:] = q[:, 64:].float().mean(0).sign().to(BF16) * 8   # head 1: one key that dominates most queries
    _check(hip, q, k, v, 1, 2, lq, lk)


def test_bindings_identical(hip):
    be = ops.backend()
    if getattr(be, "binding", "ctypes") != "torch":
        pytest.skip("the torch.ops binding is not loaded on this host")
    q, k, v = _qkv(2, 5, 640, 640, seed=21, fused=True)
    a = hip.attention_q8(q, k, v, batch=2, heads=5, lq=640, lk=640, scale=0.125)
    b = be.attention_q8(q, k, v, batch=2, heads=5, lq=640, lk=640, scale=0.125)
    assert torch.equal(a, b)


def test_operands_at_allocation_end(hip):
    """q, k, v, the output and the workspace each end exactly where their hipMalloc region ends."""
    batch, heads, lq, lk = 1, 2, 77, 33
    hd = heads * 64
    regs = []

    def carve(n_rows, cols, src=None):
        r = _Region(n_rows * cols * 2, (n_rows, cols), "<i2")
        regs.append(r)
        t = torch.as_tensor(r, device=DEV).view(BF16)
        if src is not None:
            t.copy_(src)
        return t

    q0, k0, v0 = _qkv(batch, heads, lq, lk, seed=9)
    q, k, v, o = carve(lq, hd, q0), carve(lk, hd, k0), carve(lk, hd, v0), carve(lq, hd)
    p = hip._q8_params(q, k, v, o, batch, heads, lq, lk, 0.125)
    nbytes = hip.lib.tc_attn_q8_workspace(C.byref(p))
    wr = _Region(nbytes, (nbytes,), "|u1")
    regs.append(wr)
    p.workspace, p.workspace_bytes = wr.ptr, nbytes
    _lib.check(hip.lib.tc_attn_q8_quant_kv(C.byref(p), 0), "tc_attn_q8_quant_kv")
    _lib.check(hip.lib.tc_attn_d64_q8(C.byref(p), 0), "tc_attn_d64_q8")
    torch.cuda.synchronize()
    want = hip.attention_q8(q0, k0, v0, batch=batch, heads=heads, lq=lq, lk=lk, scale=0.125)
    assert torch.equal(o, want)
    p.workspace_bytes = nbytes - 1
    assert hip.lib.tc_attn_d64_q8(C.byref(p), 0) == -4                 # TC_EWORKSPACE, nothing launched
    del q, k, v, o
    torch.cuda.synchronize()


def test_graph_replay_equals_eager(hip):
    q, k, v = _qkv(2, 5, 640, 640, seed=13, fused=True)
    eager = hip.attention_q8(q, k, v, batch=2, heads=5, lq=640, lk=640, scale=0.125)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.attention_q8(q, k, v, batch=2, heads=5, lq=640, lk=640, scale=0.125)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.attention_q8(q, k, v, batch=2, heads=5, lq=640, lk=640, scale=0.125)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
