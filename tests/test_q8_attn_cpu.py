"""The 8-bit spatial self-attention (ABI 14) without a GPU: the CPU restatement (tests/q8_attn_ref.py) is softmax attention
when its quantisers are the identity, the quantisers keep their invariants, the format choice (int8 q k^T, MXFP8 P v) is
pinned by its error against the alternatives, the ABI / ctypes struct / torch op agree with the header, the routing rule
is host logic, and the kernel compiles with both new MFMA forms and no scratch."""
import ctypes as C
import os
import re

import pytest
import torch

import q8_attn_ref as R
from oracle import mx
from test_isa_cpu import _asm, _kernels
from tooncrafter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("lq,lk", [(50, 1000), (33, 77), (64, 33), (7, 128)])
def test_identity_quantisers_give_softmax_attention(lq, lk):
    g = torch.Generator().manual_seed(lq * lk)
    q, k, v = (torch.randn(n, 64, generator=g, dtype=torch.float64) * 2 for n in (lq, lk, lk))
    got = R.attention(q, k, v, 0.125, qk=None, pv_mx=False, dtype=torch.float64)
    want = R.softmax_attention(q, k, v, 0.125)
    assert (got - want).abs().max().item() <= 1e-12


def test_int8_row_quantiser_invariants():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(300, 64, generator=g) * torch.logspace(-3, 2, 300)[:, None]).to(torch.bfloat16).float()
    x[7] = 0
    q, s = R.quant_rows_i8(x)
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    assert int(q.abs().max()) == 127 and (q != -128).all()
    assert (q[7] == 0).all() and s[7] == 1.0
    nz = torch.arange(300) != 7
    assert (q[nz].abs().amax(dim=1) == 127).all()                       # the row amax maps to +-127
    err = (q.float() * s[:, None] - x).abs() / s[:, None]
    assert err.max() <= 0.5 + 1e-5                                      # round to nearest on the row grid


def test_vt_mx_quantiser_is_the_mx_oracle():
    g = torch.Generator().manual_seed(2)
    v = torch.randn(77, 64, generator=g).to(torch.bfloat16).float()
    vq, vs = R.quant_vt_mx(v)
    assert vq.shape == (64, 128) and vs.shape == (64, 4)
    vt = torch.zeros(64, 128)
    vt[:, :77] = v.t()
    q2, s2 = mx.quantize_mxfp8(vt)
    assert torch.equal(vq, q2) and torch.equal(vs, s2)
    assert (vq[:, 77:] == 0).all()                                       # padded keys: zero bytes (e4m3 +0)


def test_records_hold_the_quantised_operands():
    g = torch.Generator().manual_seed(3)
    k, v = (torch.randn(100, 64, generator=g).to(torch.bfloat16).float() for _ in range(2))
    rec = R.pack_records(k, v)
    assert rec.shape == (2, R.REC)
    kq, ks = R.quant_rows_i8(k)
    # fragment 2 kbk + kk, lane L: key 32 kbk + (L & 31), dims 32 kk + 16 (L >> 5) ..
    frag = rec[1, 1 * 1024:2 * 1024].view(torch.int8).view(64, 16)          # tile 1, kbk 0, kk 1
    assert torch.equal(frag[5], kq[64 + 5, 32:48]) and torch.equal(frag[32 + 3], kq[64 + 3, 48:64])
    assert (rec[1, 2 * 1024:3 * 1024].view(64, 16)[[4 + i for i in range(28)] + [36 + i for i in range(28)]] == 0).all()  # keys >= lk
    assert torch.equal(rec[0, 8192:8448].view(torch.float32), ks[:64])
    assert (rec[1, 8192:8448].view(torch.float32)[36:] == 0).all()         # keys past lk: scale 0


def test_format_choice_pinned_at_full_length():
    """sigma = 2, L = 2560, d = 64, scale 1/8, MX P.V in every arm: int8-row q k^T stays within 1.3x of bf16 q k^T,
    MXFP8-e4m3 q k^T is at least 2x it (the estimate that chose the format: 1.1x and 3.2x)."""
    g = torch.Generator().manual_seed(0)
    L = 2560
    q = (torch.randn(L, 64, generator=g) * 2).to(torch.bfloat16).float()
    k = (torch.randn(L, 64, generator=g) * 2).to(torch.bfloat16).float()
    v = torch.randn(L, 64, generator=g).to(torch.bfloat16).float()
    ref = R.softmax_attention(q, k, v, 0.125)
    e = {arm: _rel(R.attention(q, k, v, 0.125, qk=arm), ref) for arm in ("int8", "bf16", "mx")}
    print("rel-L2 vs fp64 attention:", {a: f"{x:.3e}" for a, x in e.items()})
    assert e["int8"] <= 1.3 * e["bf16"]
    assert e["mx"] >= 2.0 * e["bf16"]


def test_abi_14_and_struct_layout():
    assert _lib.TC_ABI_VERSION == 14
    lib = _lib.load()
    assert lib.tc_abi_version() == 14
    for name in ("tc_attn_q8_workspace", "tc_attn_q8_quant_kv", "tc_attn_d64_q8"):
        assert name in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "tooncrafter_hip.h")) as f:
        hdr = f.read()
    body = re.search(r"typedef struct TcAttnQ8Params \{(.*?)\} TcAttnQ8Params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *rest = decl.split(",")
        names += [re.split(r"[\s*]+", first.strip())[-1]] + [r.strip() for r in rest]
    assert names == [f[0] for f in _lib.TcAttnQ8Params._fields_]


def test_quant_kv_validation_without_launch():
    lib = _lib.load()
    p = _lib.TcAttnQ8Params()
    assert lib.tc_attn_q8_quant_kv(C.byref(p), None) == -1               # TC_EINVAL: nothing set
    p.batch, p.heads, p.lq, p.lk, p.scale = 2, 5, 2560, 2560, 0.125
    assert lib.tc_attn_q8_workspace(C.byref(p)) == 2 * 5 * 40 * R.REC
    p.q = p.k = p.v = p.o = p.workspace = 0x1000
    p.q_ss = p.k_ss = p.v_ss = p.o_ss = 960
    p.workspace_bytes = 2 * 5 * 40 * R.REC - 1
    assert lib.tc_attn_q8_quant_kv(C.byref(p), None) == -4               # TC_EWORKSPACE
    p.k_ss = 962
    assert lib.tc_attn_q8_quant_kv(C.byref(p), None) == -2               # TC_EALIGN
    p.k_ss, p.scale = 960, 0.0
    assert lib.tc_attn_d64_q8(C.byref(p), None) == -1                    # scale must be > 0


def test_torch_op_schema_and_meta():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    schema = str(t.attention_q8.default._schema)
    assert schema == ("tooncrafter::attention_q8(Tensor q, Tensor k, Tensor v, int batch, int heads, int lq, int lk, "
                      "float scale) -> Tensor"), schema
    bf = dict(dtype=torch.bfloat16, device="meta")
    qkv = torch.empty(32 * 2560, 3 * 320, **bf)
    y = t.attention_q8(qkv[:, :320], qkv[:, 320:640], qkv[:, 640:], 32, 5, 2560, 2560, 0.125)
    assert y.shape == (32 * 2560, 320) and y.dtype == torch.bfloat16


def test_routing_rule_is_host_logic(monkeypatch):
    from tooncrafter_amd.ops import HipOps
    monkeypatch.delenv("TC_FP8_ATTN", raising=False)
    monkeypatch.delenv("TC_FP8_ATTN_MIN_LK", raising=False)
    h = HipOps()
    assert h.fp8_attn is False and h.fp8_attn_min_lk == 640 and h.fp8_calls["attn_q8"] == 0
    assert not h.spatial_attn_q8_eligible(lk=2560)                         # off by default
    h.fp8_attn = True
    assert h.spatial_attn_q8_eligible(lk=2560) and h.spatial_attn_q8_eligible(lk=640)
    assert not h.spatial_attn_q8_eligible(lk=160)                          # levels 2 / 3
    assert not h.spatial_attn_q8_eligible(lk=2560, k2=object())            # text + image cross-attention
    assert not h.spatial_attn_q8_eligible(lk=2560, accumulate=True)
    assert not h.spatial_attn_q8_eligible(lk=2560, kv_bdiv=16)
    monkeypatch.setenv("TC_FP8_ATTN", "1")
    monkeypatch.setenv("TC_FP8_ATTN_MIN_LK", "2560")
    h2 = HipOps()
    assert h2.fp8_attn and h2.spatial_attn_q8_eligible(lk=2560) and not h2.spatial_attn_q8_eligible(lk=640)


def test_emulation_backend_has_no_q8_route():
    from emu_ops import EmuOps
    assert not hasattr(EmuOps(round_bf16=False), "spatial_attn_q8_eligible")


def test_isa_both_mfma_forms_no_scratch(tmp_path_factory):
    asm = _asm(tmp_path_factory, "attention_q8")
    ks = _kernels(asm)
    attn = [b for n, b in ks.items() if "attn_d64_q8_kernel" in n]
    assert len(attn) == 1
    assert "v_mfma_i32_32x32x32_i8" in attn[0] and "v_mfma_scale_f32_32x32x64_f8f6f4" in attn[0]
    assert "v_cvt_pk_fp8_f32" in attn[0]
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", asm):
        assert int(m.group(1)) == 0, "a kernel of attention_q8.hip spills to scratch"
