"""Every attention kernel against the bit-exact expectations of tests/attn_exact_cases.py, on the MI355X.

A case's inputs make the correct output known to the bit (attention as a gather: the output row IS a chosen V row; equal
weights: every valid key counted exactly once): torch.equal through attn_exact_cases.differences, no tolerance.  The
expectation is a float64 computation on the CPU that test_attn_exact_cpu.py holds to its closed form and to the seeded
defects; it shares no code with tests/emu_ops.py.  Outputs the caller allocates are slices of sentinel-filled buffers with
sentinel rows behind them, and nothing beside or behind the output may change.

A failure names the kernel, counts the differing outputs, lists the first few (batch, head, query, dim, got, want), gives
the residues of the differing queries modulo 32 and 128 and of their target keys modulo 4 .. 64, and for a gather case says
which key's V row arrived instead: a permutation, a tile edge or a batch mapping shows in those."""
import os
import subprocess
import sys

import pytest
import torch

import attn_exact_cases as X

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
PAD_ROWS = 37


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def expected():
    """name -> (inputs, stored expectation): computed once, on the CPU, never modified"""
    cache = {}

    def get(c):
        if c.name not in cache:
            inp = X.inputs(c)
            cache[c.name] = (inp, X.expected(c, inp))
        return cache[c.name]
    return get


def _dev(x):
    return x.to(BF16).to(DEV)


def _sentinels(shape):
    return torch.full(shape, X.SENTINEL, dtype=BF16, device=DEV)


def run_attention(h, c, inp):
    """ops.attention on a spatial case -> the output's whole buffer: [rows + PAD_ROWS, C] with the output in its first rows,
    or (packed) [rows + PAD_ROWS, 3 C] with the output in the middle column block and q, k, v column slices of one buffer"""
    cw, rows = c.heads * X.D, c.batch * c.lq
    if c.packed:
        assert c.lq == c.lk and c.kv_bdiv == 1
        qkv = _dev(torch.cat([inp["q"], inp["k"], inp["v"]], 1))
        q, k, v = qkv[:, :cw], qkv[:, cw:2 * cw], qkv[:, 2 * cw:]
        buf = _sentinels((rows + PAD_ROWS, 3 * cw))
        out = buf[:rows, cw:2 * cw]
    else:
        q, k, v = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"])
        buf = _sentinels((rows + PAD_ROWS, cw))
        out = buf[:rows]
    if c.accumulate:
        out.copy_(_dev(inp["base"]))
    kw = dict(batch=c.batch, heads=c.heads, lq=c.lq, lk=c.lk, kv_bdiv=c.kv_bdiv, out=out, accumulate=c.accumulate)
    if c.lk2:
        kw.update(k2=_dev(inp["k2"]), v2=_dev(inp["v2"]), lk2=c.lk2, kv2_bdiv=c.kv2_bdiv)
    h.attention(q, k, v, **kw)
    torch.cuda.synchronize()
    return buf


def judge_attention(c, buf, inp, want, what=""):
    cw, rows = c.heads * X.D, c.batch * c.lq
    buf = buf.cpu()
    out = buf[:rows, cw:2 * cw] if c.packed else buf[:rows]
    report = X.differences(c, out, want, inp)
    assert report is None, what + report
    s = X.SENTINEL
    assert bool((buf[rows:] == s).all()), f"{what}{c.name} [{c.target}]: rows behind the output were written"
    if c.packed:
        assert bool((buf[:rows, :cw] == s).all()) and bool((buf[:rows, 2 * cw:] == s).all()), \
            f"{what}{c.name} [{c.target}]: columns beside the output slice were written"


SPATIAL = [c for c in X.CASES if c.op == "attention"]


@pytest.mark.parametrize("c", SPATIAL, ids=lambda c: c.name)
def test_attention(c, hip, expected):
    inp, want = expected(c)
    judge_attention(c, run_attention(hip, c, inp), inp, want)


_REG_CHILD = """
import sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import attn_exact_cases as X
import test_gpu_attn_exact as t
from tooncrafter_amd.ops import HipOps
hip, outs = HipOps(), {}
for c in X.REG_CASES:
    outs[c.name] = t.run_attention(hip, c, X.inputs(c)).cpu()
torch.save(outs, sys.argv[2])
"""


@pytest.fixture(scope="module")
def reg_outputs(tmp_path_factory):
    """TC_ATTN_STAGE=reg (attn_d64_kernel) is latched at a process's first attention call: the non-dual cases run in ONE fresh
    child process, the buffers are judged here"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path_factory.mktemp("attn_exact") / "reg.pt"
    r = subprocess.run([sys.executable, "-c", _REG_CHILD, root, str(path)], capture_output=True, text=True,
                       env=dict(os.environ, TC_ATTN_STAGE="reg"), timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return torch.load(path)


@pytest.mark.parametrize("c", X.REG_CASES, ids=lambda c: c.name)
def test_attention_register_staged(c, reg_outputs, expected):
    inp, want = expected(c)
    assert c.name in reg_outputs
    judge_attention(c, reg_outputs[c.name], inp, want, what="attn_d64_kernel (TC_ATTN_STAGE=reg): ")


@pytest.mark.parametrize("c", [c for c in X.CASES if c.op == "attention_q8"], ids=lambda c: c.name)
def test_attention_q8(c, hip, expected):
    inp, want = expected(c)
    out = hip.attention_q8(_dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"]), batch=c.batch, heads=c.heads, lq=c.lq, lk=c.lk)
    torch.cuda.synchronize()
    report = X.differences(c, out.cpu(), want, inp)
    assert report is None, report


@pytest.mark.parametrize("c", [c for c in X.CASES if c.op in ("temporal", "temporal_rel")], ids=lambda c: c.name)
def test_attention_temporal(c, hip, expected):
    inp, want = expected(c)
    kw = dict(b=c.batch, t=c.t, hw=c.hw, heads=c.heads)
    if c.op == "temporal":
        out = hip.attention_temporal(_dev(inp["qkv"]), **kw)
    else:
        rel_k, rel_v = (_dev(inp["rel_k"]), _dev(inp["rel_v"])) if c.tables else (None, None)
        out = hip.attention_temporal_rel(_dev(inp["qkv"]), rel_k, rel_v, max_rel=c.max_rel, causal=int(c.causal), **kw)
    torch.cuda.synchronize()
    report = X.differences(c, out.cpu(), want, inp)
    assert report is None, report


def _strided_x(c, inp, pitch):
    """x as the leading columns of the middle rows of a sentinel-filled [PAD_ROWS + rows + PAD_ROWS, pitch] buffer"""
    rows, cw = inp["x"].shape
    buf = _sentinels((rows + 2 * PAD_ROWS, pitch))
    x = buf[PAD_ROWS:PAD_ROWS + rows, :cw]
    x.copy_(_dev(inp["x"]))
    return x


@pytest.mark.parametrize("c", [c for c in X.CASES if c.op == "qkv_attn"], ids=lambda c: c.name)
def test_temporal_qkv_attn(c, hip, expected, monkeypatch):
    monkeypatch.setenv("TC_QKV_ATTN", "2")
    inp, want = expected(c)
    rows, cw = inp["x"].shape
    x = _strided_x(c, inp, cw + 64)
    buf = _sentinels((rows + 2 * PAD_ROWS, cw + 128))
    out = buf[PAD_ROWS:PAD_ROWS + rows, :cw]
    assert hip.temporal_qkv_attn_eligible(b=c.batch, t=c.t, hw=c.hw, c=cw, heads=c.heads, ldx=x.stride(0)), "the library refuses the shape"
    hip.temporal_qkv_attn(x, _dev(inp["wqkv"]), inp["bqkv"].float().to(DEV), b=c.batch, t=c.t, hw=c.hw, heads=c.heads, out=out)
    torch.cuda.synchronize()
    buf = buf.cpu()
    report = X.differences(c, buf[PAD_ROWS:PAD_ROWS + rows, :cw], want, inp)
    assert report is None, report
    s = X.SENTINEL
    assert bool((buf[:PAD_ROWS] == s).all()) and bool((buf[PAD_ROWS + rows:] == s).all()), f"{c.name}: rows in front of / behind the output were written"
    assert bool((buf[:, cw:] == s).all()), f"{c.name}: columns beside the output were written"


@pytest.mark.parametrize("c", [c for c in X.CASES if c.op == "tb_fused"], ids=lambda c: c.name)
def test_temporal_attn_fused(c, hip, expected, monkeypatch):
    monkeypatch.setenv("TC_TB_FUSED", "1")
    inp, want = expected(c)
    cw = c.heads * X.D
    x = _strided_x(c, inp, 3 * cw)
    assert hip.temporal_attn_fused_eligible(b=c.batch, t=c.t, hw=c.hw, c=cw, heads=c.heads, ldx=x.stride(0)), "the library refuses the shape"
    out = hip.temporal_attn_fused(x, _dev(inp["wqkv"]), inp["bqkv"].float().to(DEV), _dev(inp["wo"]), inp["bo"].float().to(DEV),
                                  b=c.batch, t=c.t, hw=c.hw, heads=c.heads, ln_eps=None)
    torch.cuda.synchronize()
    report = X.differences(c, out.cpu(), want, inp)
    assert report is None, report
