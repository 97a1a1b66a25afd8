"""Temporal attention with relative position and / or a causal mask, without a GPU: the two UNet kwargs build and load the
reference's keys, the module mirror on the emulated contract reproduces the reference's outputs (golden:
tests/golden/make_relpos_golden.py), a relative / causal attention is routed to tc_attn_temporal_rel and nowhere else, the
refusals happen on the host, and the entry point is declared, exported and bound with the header's layout (ABI still 14).
Compute is covered by tests/test_gpu_relpos.py."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import relpos_cases as rc
from conftest import ROOT, TINY_UNET_CFG, load_golden, rel_l2
from tooncrafter_amd import ops

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
FIELDS = ("qkv", "out", "rel_k", "rel_v", "b", "t", "hw", "heads", "max_rel", "causal", "scale")


def _with_backend(backend, fn):
    prev = ops.set_backend(backend)
    try:
        return fn()
    finally:
        ops.set_backend(prev)


@pytest.fixture(scope="module")
def golden():
    return load_golden("unet_relpos_tiny.npz")


# ------------------------------------------------------------------------------------------------ construction, keys
def test_both_flags_build_and_load_the_reference_keys(golden):
    from tooncrafter_amd.lvdm.attention import CrossAttention, RelativePosition
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    un = UNetModel(**dict(TINY_UNET_CFG, use_relative_position=True, use_causal_attention=True))
    keys = [str(k) for k in golden["keys_both"]]
    sd = un.state_dict()
    assert set(sd) == set(keys) and len(sd) == len(keys)
    tables = [k for k in keys if k.endswith(".embeddings_table")]
    assert sorted(tables) == sorted(str(n) for n in golden["table_names"]) and len(tables) == 68
    assert all(re.search(r"\.attn[12]\.relative_position_[kv]\.embeddings_table$", k) for k in tables)
    assert all(tuple(sd[k].shape) == (9, 64) for k in tables)
    un.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)
    rel = [m for m in un.modules() if isinstance(m, CrossAttention) and m.relative_position]
    assert len(rel) * 2 == len(tables) and all(isinstance(m.relative_position_k, RelativePosition) for m in rel)
    assert not un.init_attn[0].causal_attention and un.init_attn[0].relative_position      # openaimodel3d.py:398
    # a config that leaves use_relative_position out gets the reference's default: relative
    cfg = {k: v for k, v in TINY_UNET_CFG.items() if k != "use_relative_position"}
    assert any(k.endswith(".embeddings_table") for k in UNetModel(**cfg).state_dict())
    # the remaining switch stays closed, and the table size is bounded by the kernel's
    from tooncrafter_amd.lvdm.attention import TemporalTransformer
    with pytest.raises(NotImplementedError):
        TemporalTransformer(64, 1, 64, only_self_att=False)
    with pytest.raises(ValueError):
        TemporalTransformer(64, 1, 64, relative_position=True, temporal_length=65)
    with pytest.raises(AssertionError):
        CrossAttention(64, heads=1, relative_position=True)


def test_tables_are_packed_once_and_repacked_on_new_weights():
    from tooncrafter_amd.lvdm.attention import CrossAttention
    torch.manual_seed(3)
    at = CrossAttention(64, heads=1, relative_position=True, temporal_length=4)
    pk = at.pk
    assert pk["rel_k"].dtype == torch.bfloat16 and tuple(pk["rel_k"].shape) == (9, 64) and pk["rel_k"].is_contiguous()
    assert torch.equal(pk["rel_v"], at.relative_position_v.embeddings_table.detach().to(torch.bfloat16))
    assert at.pk["rel_k"] is pk["rel_k"]
    sd = {k: v + 1 for k, v in at.state_dict().items()}
    at.load_state_dict(sd, strict=True)
    assert torch.equal(at.pk["rel_k"], sd["relative_position_k.embeddings_table"].to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ the statement itself
def test_statement_matches_a_loop_over_frames():
    """rel_attn_f64 against the formulas written out one (i, j) at a time."""
    g = torch.Generator().manual_seed(5)
    b, t, hw, heads, L = 1, 6, 2, 2, 4
    x = torch.randn(b, t, hw, 3, heads, 64, generator=g, dtype=torch.float64)
    rk, rv = (torch.randn(2 * L + 1, 64, generator=g, dtype=torch.float64) * 0.5 for _ in range(2))
    for causal in (False, True):
        got = rc.rel_attn_f64(x, rk, rv, max_rel=L, causal=causal, scale=0.125)
        for p in range(hw):
            for h in range(heads):
                q, k, v = (x[0, :, p, i, h] for i in range(3))
                for i in range(t):
                    js = [j for j in range(t) if not (causal and j > i)]
                    idx = [min(max(j - i, -L), L) + L for j in js]
                    s = torch.stack([0.125 * (q[i] @ k[j] + q[i] @ rk[r]) for j, r in zip(js, idx)])
                    w = s.softmax(0)
                    o = sum(w[n] * (v[j] + rv[r]) for n, (j, r) in enumerate(zip(js, idx)))
                    assert torch.allclose(got[0, i, p, h], o, rtol=1e-12, atol=1e-12)
    plain = rc.rel_attn_f64(x, None, None, max_rel=0, causal=False, scale=0.125)
    q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))
    assert torch.allclose(plain, (((q @ k.transpose(-1, -2)) * 0.125).softmax(-1) @ v).permute(0, 3, 1, 2, 4), rtol=1e-12)


# ------------------------------------------------------------------------------------------------ tiny UNet vs golden
@pytest.mark.parametrize("variant", list(rc.VARIANTS))
def test_tiny_unet_on_the_emulated_contract_vs_reference_golden(golden, variant):
    """The mirror on RelEmuOps against the reference's fp32 output.  The figure is the contract's own error for this
    variant: relpos_cases.UNET_CONTRACT records it (it decides the bound of the GPU test) and this test re-measures it."""
    un = rc.tiny_unet(variant)
    if rc.VARIANTS[variant][0]:
        rc.set_tables(un, golden)
    args, kw = rc.unet_inputs(golden, variant)
    emu = rc.RelEmuOps()
    with torch.no_grad():
        y = _with_backend(emu, lambda: un(*args, **kw))
    ref = torch.from_numpy(golden["y_" + variant])
    e = rel_l2(y, ref)
    t = rc.VARIANTS[variant][2]
    d = rel_l2(y, torch.from_numpy(golden[f"y_plain{t}"]))
    print(f"tiny UNet {variant} on the emulated contract vs reference golden: {e:.3e}; distance to the flagless output {d:.3e}")
    assert torch.isfinite(y).all() and emu.rel_calls > 0
    assert abs(e - rc.UNET_CONTRACT[variant]) <= 0.02 * rc.UNET_CONTRACT[variant], (e, rc.UNET_CONTRACT[variant])
    assert e < rc.unet_bound(variant) < d                                # a missing term cannot pass
    assert float(golden["d_" + variant]) >= 1e-1


def test_flagless_tiny_unet_matches_the_fixture_too(golden):
    """The fixture's flagless outputs are the model every variant is measured against: the mirror reproduces them."""
    un = rc.tiny_unet()
    emu = rc.RelEmuOps()
    for t in (4, 6):
        args, kw = rc.unet_inputs(golden, t)
        with torch.no_grad():
            y = _with_backend(emu, lambda: un(*args, **kw))
        assert rel_l2(y, torch.from_numpy(golden[f"y_plain{t}"])) < rc.UNET_BORROWED
    assert emu.rel_calls == 0


# ------------------------------------------------------------------------------------------------ routing
class Recorder(rc.RelEmuOps):
    """Offers every fused temporal route (the one-launch qkv + attention, the LayerNorm fold of the projection) and
    records what is called."""

    def __init__(self, **k):
        super().__init__(**k)
        self.seq, self.depth = [], 0

    def temporal_qkv_attn_eligible(self, **k):
        return True

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name in ("gemm", "attention", "attention_temporal", "attention_temporal_rel", "temporal_qkv_attn",
                    "temporal_attn_fused", "ff_geglu_fused", "layernorm", "groupnorm"):
            seq = object.__getattribute__(self, "seq")

            def wrapped(*a, _v=v, _n=name, **kw):
                if self.depth == 0:              # what the model calls; an emulated fused operator calls others inside
                    seq.append(_n if _n != "gemm" else "gemm_ln" if kw.get("a_norm_eps") is not None else "gemm")
                self.depth += 1
                try:
                    return _v(*a, **kw)
                finally:
                    self.depth -= 1
            return wrapped
        return v


def _blocks(un):
    from tooncrafter_amd.lvdm.attention import TemporalTransformer
    return sum(len(m.transformer_blocks) for m in un.modules() if isinstance(m, TemporalTransformer))


@pytest.mark.parametrize("variant", ["rel", "causal", "both"])
def test_relative_or_causal_attention_takes_the_projection_and_the_new_kernel(golden, variant):
    un = rc.tiny_unet(variant)
    args, kw = rc.unet_inputs(golden, variant)
    for extra in (dict(), dict(ln_fusion_k=64), dict(tb_fused_c=64)):
        rec = Recorder(**extra)
        with torch.no_grad():
            _with_backend(rec, lambda: un(*args, **kw))
        n = _blocks(un)
        assert n == 17
        # init_attn is never causal: under "causal" its block (512 wide) is a flagless one and keeps the one-launch route
        n_rel = n if variant != "causal" else n - 1
        assert rec.seq.count("temporal_qkv_attn") == 2 * (n - n_rel) and rec.seq.count("temporal_attn_fused") == 0
        assert rec.seq.count("attention_temporal_rel") == 2 * n_rel and rec.rel_calls == 2 * n_rel
        assert rec.seq.count("attention_temporal") == 0
        # every call is the projection, the attention, the output projection; the LayerNorm fold still applies
        before = [rec.seq[i - 1] for i, name in enumerate(rec.seq) if name == "attention_temporal_rel"]
        after = [rec.seq[i + 1] for i, name in enumerate(rec.seq) if name == "attention_temporal_rel"]
        assert set(before) <= {"gemm", "gemm_ln"} and set(after) == {"gemm"}
        # the fold is offered at K = 64 only: the one-head blocks of level 0 take it, the others a LayerNorm
        assert before.count("gemm_ln") == (2 * sum(len(m.transformer_blocks) for m in un.modules()
                                                   if type(m).__name__ == "TemporalTransformer" and m.transformer_blocks[0].attn1.heads == 1
                                                   and (m.causal_attention or m.relative_position))
                                           if extra.get("ln_fusion_k") else 0)
        assert not extra.get("ln_fusion_k") or before.count("gemm_ln") > 0


# sha256 of the flagless model's operator sequence under Recorder() / Recorder(tb_fused_c=64), taken on the commit before
# tc_attn_temporal_rel existed: models without the two flags take exactly the routes they took
FLAGLESS_SEQ = {"plain": "01206f24bf338b2d3770e3daaa59feeaf78ef4d752857f325bfd363be2efe0f3", "tb_fused": "549fa7141b3c1e6a847fa711c0d07a951c0d4149027ef24bfb472a38047e5f52"}


def test_flagless_model_takes_the_routes_it_took(golden):
    un = rc.tiny_unet()
    args, kw = rc.unet_inputs(golden, 4)
    for tag, extra in (("plain", dict()), ("tb_fused", dict(tb_fused_c=64))):
        rec = Recorder(**extra)
        with torch.no_grad():
            _with_backend(rec, lambda: un(*args, **kw))
        n = _blocks(un)
        assert rec.rel_calls == 0 and rec.seq.count("attention_temporal") == 0
        if tag == "plain":
            assert rec.seq.count("temporal_qkv_attn") == 2 * n
        else:
            assert rec.seq.count("temporal_attn_fused") > 0
        digest = hashlib.sha256(" ".join(rec.seq).encode()).hexdigest()
        print(tag, len(rec.seq), digest)
        assert digest == FLAGLESS_SEQ[tag]


# ------------------------------------------------------------------------------------------------ host refusals
class NoOps:
    """A backend with no operators: any launch is an AttributeError."""
    name = "none"


def test_causal_clip_longer_than_the_mask_is_refused_before_any_op(golden):
    un = rc.tiny_unet("causal")
    (x, ts), kw = rc.unet_inputs(golden, 6)                              # 6 frames, temporal_length 4
    with pytest.raises(ValueError, match="temporal_length"):
        _with_backend(NoOps(), lambda: un(x, ts, **kw))
    rel = rc.tiny_unet("rel")                                            # relative only: distances clamp, 6 frames run
    with pytest.raises(AttributeError):
        _with_backend(NoOps(), lambda: rel(x, ts, **kw))
    from tooncrafter_amd.lvdm.attention import TemporalTransformer
    from tooncrafter_amd.lvdm.common import Act
    tt = TemporalTransformer(64, 1, 64, causal_attention=True, temporal_length=4)
    with pytest.raises(ValueError, match="temporal_length"):
        _with_backend(NoOps(), lambda: tt(Act(torch.zeros(5 * 2, 64, dtype=torch.bfloat16), 1, 5, 1, 2)))


def test_header_declares_the_entry_point_and_abi_is_unchanged():
    from tooncrafter_amd import _lib
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"\bint\s+tc_attn_temporal_rel\s*\(\s*const\s+TcAttnTemporalRelParams\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"#define\s+TC_ABI_VERSION\s+14\b", header) and _lib.TC_ABI_VERSION == 14
    doc = header[header.index("relative position and / or a causal mask"):header.index("typedef struct TcAttnTemporalRelParams")]
    for cite in ("attention.py:20-39", "103-124", "343-345", "376-390", "TC_EINVAL", "TC_ESHAPE"):
        assert cite in doc, cite
    with open(os.path.join(ROOT, "tooncrafter_amd", "csrc", "torch_ops.cpp")) as f:
        cpp = f.read()
    assert "attention.py:20-39" in cpp and "376-390" in cpp


def test_ctypes_struct_matches_the_compiled_header(tmp_path):
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcAttnTemporalRelParams._fields_) == FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    src = tmp_path / "probe.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%zu %d", sizeof(TcAttnTemporalRelParams), TC_ABI_VERSION);']
    lines += [f'  printf(" %zu", offsetof(TcAttnTemporalRelParams, {f}));' for f in FIELDS]
    lines += ['  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.TcAttnTemporalRelParams) and got[1] == 14
    assert got[2:] == [getattr(_lib.TcAttnTemporalRelParams, f).offset for f in FIELDS]


def test_library_exports_and_binds_the_symbol():
    from tooncrafter_amd import _lib, build
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    assert hasattr(lib, "tc_attn_temporal_rel")
    res, args = _lib.SYMBOLS["tc_attn_temporal_rel"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.TcAttnTemporalRelParams), ctypes.c_void_p]
    assert _lib.load().tc_abi_version() == 14
    from tooncrafter_amd.ops import HipOps
    assert callable(HipOps.attention_temporal_rel)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every refusal returns before the launch, so it can be exercised on host pointers."""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15

    def call(**kw):
        p = _lib.TcAttnTemporalRelParams(qkv=base, out=base + 256, rel_k=base + 512, rel_v=base + 640, b=1, t=4, hw=1, heads=1,
                                         max_rel=4, causal=0, scale=0.125)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_attn_temporal_rel(ctypes.byref(p), None)
    assert lib.tc_attn_temporal_rel(None, None) == -1
    assert call(qkv=None) == -1 and call(out=None) == -1 and call(t=0) == -1 and call(heads=0) == -1 and call(scale=0.0) == -1
    assert call(rel_k=None) == -1 and call(rel_v=None) == -1                           # exactly one table
    assert call(t=65) == -3 and call(t=65, rel_k=None, rel_v=None) == -3
    assert call(max_rel=0) == -3 and call(max_rel=65) == -3 and call(max_rel=-1) == -3
    assert call(qkv=base + 2) == -2 and call(rel_v=base + 648) == -2


def test_meta_op_infers_shape_and_dtype():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    schema = str(t.attention_temporal_rel.default._schema)
    assert schema.startswith("tooncrafter::attention_temporal_rel(Tensor qkv, Tensor? rel_k, Tensor? rel_v, int b, int t, int hw, "
                             "int heads, int max_rel, bool causal, float scale)")
    qkv = torch.empty(2 * 6 * 7, 3 * 5 * 64, dtype=torch.bfloat16, device="meta")
    tab = torch.empty(9, 64, dtype=torch.bfloat16, device="meta")
    for tabs in ((tab, tab), (None, None)):
        o = t.attention_temporal_rel(qkv, *tabs, 2, 6, 7, 5, 4, True, 0.125)
        assert tuple(o.shape) == (2 * 6 * 7, 5 * 64) and o.dtype == torch.bfloat16 and o.device.type == "meta"
    with pytest.raises((RuntimeError, NotImplementedError)):            # no CPU kernel: no fallback
        c = torch.zeros(4, 192, dtype=torch.bfloat16)
        t.attention_temporal_rel(c, None, None, 1, 4, 1, 1, 4, True, 0.125)
