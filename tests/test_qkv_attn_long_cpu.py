"""tc_temporal_qkv_attn beyond 16 frames (csrc/qkv_attn_long.hip) without a GPU: the eligibility rule of the loaded library
(host code), the kernel source compiled for gfx950 -- both padded lengths, no scratch, two blocks per CU -- and the emulated
contract on the exact-data case the GPU test runs."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from emu_ops import EmuOps
from tooncrafter_amd import _lib
from tooncrafter_amd.lvdm.common import pack_linear

CSRC = os.path.join(ROOT, "tooncrafter_amd", "csrc")
BF16 = torch.bfloat16


def _eligible(t, hw, c, heads, b=2, ldx=None):
    p = _lib.TcTqaParams()
    p.b, p.t, p.hw, p.c, p.heads, p.ldx, p.ldo = b, t, hw, c, heads, c if ldx is None else ldx, c
    p.scale = 0.125
    return bool(_lib.load().tc_temporal_qkv_attn_eligible(ctypes.byref(p)))


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_16_frame_answers_are_unchanged(monkeypatch, mode):
    monkeypatch.setenv("TC_QKV_ATTN", mode)
    on = mode != "0"
    assert _eligible(16, 640, 640, 10) == on and _eligible(16, 8, 64, 1) == on and _eligible(16, 2560, 320, 5, ldx=328) == on
    assert not _eligible(16, 636, 640, 10) and not _eligible(16, 4, 640, 10)                 # hw % 8
    assert not _eligible(16, 640, 640, 8) and not _eligible(16, 640, 640, 10, ldx=636)
    assert not _eligible(8, 640, 640, 10) and not _eligible(15, 640, 640, 10)


def test_mode_2_takes_every_shape_of_the_kernel(monkeypatch):
    monkeypatch.setenv("TC_QKV_ATTN", "2")
    assert _eligible(32, 160, 1280, 20) and _eligible(32, 4, 64, 1) and _eligible(64, 2, 64, 1)
    for t in range(17, 65):
        px = 128 // (32 if t <= 32 else 64)
        for hw in (1, 2, 3, 4, 6, 8, 40, 42, 52, 2560):
            for c, heads in ((320, 5), (640, 10), (640, 8), (1280, 20), (96, 1)):
                assert _eligible(t, hw, c, heads) == (hw % px == 0 and c == heads * 64), (t, hw, c, heads)
    assert not _eligible(65, 640, 640, 10) and not _eligible(15, 640, 640, 10) and not _eligible(0, 640, 640, 10)
    assert not _eligible(32, 640, 640, 10, ldx=636) and not _eligible(32, 640, 640, 10, ldx=644)   # pitch >= c, % 8
    assert _eligible(32, 640, 640, 10, ldx=1920)
    assert not _eligible(64, 2560 * 400, 640, 10)                                            # per-lane offsets past 31 bits
    assert not _eligible(32, 640, 640, 10, b=0)


def test_mode_1_admits_only_the_cells_that_measured_ahead(monkeypatch):
    """The default: profiles/r09_qkv_attn_long_bench.txt had the one launch ahead at C = 320 / 640 for t = 24, 32, 48, 64 and
    at C = 1280 for t = 32, 64 only; lengths below a cell's lowest measured t (more padding), lengths between a losing and
    a winning t, and widths that were not measured stay on the two launches."""
    monkeypatch.setenv("TC_QKV_ATTN", "1")
    for t in range(17, 65):
        tt = 32 if t <= 32 else 64
        for c, hw in ((320, 2560), (640, 640)):
            assert _eligible(t, hw, c, c // 64) == (t >= tt * 3 // 4), (t, c)
        for hw in (160, 40):
            assert _eligible(t, hw, 1280, 20) == (t in (32, 64)), t
        for c in (64, 192, 256, 960):
            assert not _eligible(t, 640, c, c // 64), (t, c)
    assert not _eligible(32, 6, 640, 10) and not _eligible(64, 5, 640, 10)                   # the kernel's own rule still holds
    monkeypatch.delenv("TC_QKV_ATTN")
    assert _eligible(32, 640, 640, 10) and not _eligible(23, 640, 640, 10)                   # unset = 1


def test_mode_0_takes_nothing(monkeypatch):
    monkeypatch.setenv("TC_QKV_ATTN", "0")
    for t in (16, 17, 24, 32, 48, 64):
        assert not _eligible(t, 640, 640, 10)


def _hipcc():
    from tooncrafter_amd import build
    try:
        return build._hipcc()
    except RuntimeError:
        return None


def test_long_qkv_attn_kernels_compile_without_scratch(tmp_path):
    """csrc/qkv_attn_long.hip, both padded lengths (TT = 32, 64), with build.py's flags for that file: no scratch, 80 KiB
    of LDS (two blocks per CU on 160 KiB), the 32x32x16 MFMA in the code."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not on this host")
    from tooncrafter_amd import build
    assert "qkv_attn_long.hip" in build.SOURCES
    out = tmp_path / "qkv_attn_long.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", f"-I{ROOT}/include", f"-I{CSRC}",
           *build.EXTRA_FLAGS.get("qkv_attn_long.hip", []), "-S", "--cuda-device-only",
           os.path.join(CSRC, "qkv_attn_long.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    kernels = re.findall(r"^(_Z\w*qkv_attn_long_kernel\w*):", asm, re.M)
    assert len(kernels) == 2, kernels
    assert any("ILi32E" in k for k in kernels) and any("ILi64E" in k for k in kernels)
    sizes = re.findall(r"^; ScratchSize: (\d+)", asm, re.M)
    assert len(sizes) == 2 and all(int(s) == 0 for s in sizes), sizes
    lds = re.findall(r"^; LDSByteSize: (\d+)", asm, re.M)
    assert len(lds) == 2 and all(0 < int(s) <= 81920 for s in lds), lds
    occ = re.findall(r"^; Occupancy: (\d+)", asm, re.M)
    assert len(occ) == 2 and all(int(s) >= 2 for s in occ), occ
    assert "v_mfma_f32_32x32x16_bf16" in asm and "buffer_load_dwordx4" in asm and "global_store_dwordx4" in asm


def exact_case(t, hw=4, heads=3, seed=61):
    """Selector weights and one-hot softmaxes: every head's to_q copies columns 0..63 of x, to_k 64..127, to_v 128..191.
    Row (f, p) has x[sigma(f)] = 64 and x[64 + f] = 64, sigma(f) = (5 f + 3) mod t, and a random bf16 payload in columns
    128..: q_f . k_f' / 8 is 512 at f' = sigma(f) and 0 elsewhere, exp(-512) is 0 in fp32, so out[(f, p), head h] is the
    payload of frame sigma(f) of pixel p, bit for bit.  Returns x, packed wqkv, expected out (CPU)."""
    c = heads * 64
    assert c == 192 and t <= 64
    raw = torch.zeros(3 * c, c)
    j = torch.arange(64)
    for part in range(3):
        for h in range(heads):
            raw[part * c + h * 64 + j, part * 64 + j] = 1.0
    x = torch.zeros(t, hw, c)
    f = torch.arange(t)
    sigma = (5 * f + 3) % t
    x[f, :, sigma] = 64.0
    x[f, :, 64 + f] = 64.0
    x[:, :, 128:] = torch.randn(t, hw, 64, generator=torch.Generator().manual_seed(seed))
    x = x.to(BF16)
    want = x[sigma][:, :, 128:].repeat(1, 1, heads)
    return x.reshape(t * hw, c), pack_linear(raw), want.reshape(t * hw, c)


def test_emulated_contract_gives_the_exact_result_at_24_frames():
    x, w, want = exact_case(24)
    got = EmuOps(round_bf16=True, tqa=True).temporal_qkv_attn(x, w, None, b=1, t=24, hw=4, heads=3)
    assert got.dtype == BF16 and torch.equal(got.view(torch.int16), want.view(torch.int16))
