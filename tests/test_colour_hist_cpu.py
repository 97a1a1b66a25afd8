"""Histogram colour transfer, everything that needs no GPU: the declaration, layout and export of the C ABI (tc_colour_hist,
tc_colour_transfer), the Meta kernels, every refusal (before any launch, so host pointers do), the numpy statement of
tests/colour_hist_ref.py on its own (edge bins, the exact consequences, the rank bracket in separate integer arithmetic, the
seeds of the compound's GPU test), the wiring of the two new `match=` methods through the synthesis calls on a recording
backend, and the compile of csrc/colour_hist.hip without scratch."""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import colour_hist_ref as ref
import colour_match_ref as cm
from conftest import ROOT
from test_colour_match_cpu import Spy

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
HIST_FIELDS = ("x", "b", "t", "h", "w", "f0", "nf", "fstep", "hist", "workspace", "workspace_bytes")
TRANSFER_FIELDS = ("x", "base", "out", "b", "t", "h", "w", "src", "ref", "ref_pixels", "strength", "table")
ENTRY_POINTS = ("tc_colour_hist_workspace", "tc_colour_hist", "tc_colour_transfer")
COMPOUND_SEEDS = (0, 3)                                                          # tests/test_gpu_colour_hist.py uses these


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_and_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_colour_hist_workspace"] == (ctypes.c_int64, [ctypes.POINTER(_lib.TcColourHistParams)])
    assert _lib.SYMBOLS["tc_colour_hist"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcColourHistParams), ctypes.c_void_p])
    assert _lib.SYMBOLS["tc_colour_transfer"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcColourTransferParams), ctypes.c_void_p])
    assert _lib.load().tc_abi_version() == 14 and _lib.TC_ABI_VERSION == 14       # additive: the version stays
    assert _lib.TC_COLOUR_METHODS == {"mean_std": 0, "mkl": 1}                    # no third method code of tc_colour_match
    with open(HEADER) as f:
        header = f.read()
    assert "int64_t tc_colour_hist_workspace(const TcColourHistParams* p);" in header
    assert "int tc_colour_hist(const TcColourHistParams* p, void* stream);" in header
    assert "int tc_colour_transfer(const TcColourTransferParams* p, void* stream);" in header
    assert "#define TC_COLOUR_BINS 1024" in header
    assert "colour_hist.hip" in build.SOURCES
    for name in ("colour_hist", "colour_transfer"):
        assert callable(getattr(HipOps, name)) and getattr(TorchLibOps, name) is not getattr(HipOps, name)


def test_ctypes_structs_match_the_compiled_header(tmp_path):
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcColourHistParams._fields_) == HIST_FIELDS
    assert tuple(f[0] for f in _lib.TcColourTransferParams._fields_) == TRANSFER_FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %d %zu %zu", TC_ABI_VERSION, TC_COLOUR_BINS, sizeof(TcColourHistParams), sizeof(TcColourTransferParams));']
    lines += [f'  printf(" %zu", offsetof(TcColourHistParams, {f}));' for f in HIST_FIELDS]
    lines += [f'  printf(" %zu", offsetof(TcColourTransferParams, {f}));' for f in TRANSFER_FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [14, 1024, ctypes.sizeof(_lib.TcColourHistParams), ctypes.sizeof(_lib.TcColourTransferParams)]
    assert got[4:4 + len(HIST_FIELDS)] == [getattr(_lib.TcColourHistParams, f).offset for f in HIST_FIELDS]
    assert got[4 + len(HIST_FIELDS):] == [getattr(_lib.TcColourTransferParams, f).offset for f in TRANSFER_FIELDS]
    assert _lib.TC_COLOUR_BINS == 1024 == ref.BINS


def test_meta_kernels_infer_shapes_and_dtypes():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    assert str(t.colour_hist.default._schema) == "tooncrafter::colour_hist(Tensor x, int f0, int nf, int fstep) -> Tensor"
    assert str(t.colour_transfer.default._schema) == ("tooncrafter::colour_transfer(Tensor x, Tensor? base, Tensor src, Tensor ref, "
                                                      "int ref_pixels, float strength) -> (Tensor, Tensor)")
    x = torch.empty(2, 3, 5, 24, 40, device="meta")
    for (f0, nf, fstep) in ((0, 5, 1), (0, 2, 4), (1, 1, 1), (4, 1, 0), (1, 2, 3)):
        s = t.colour_hist(x, f0, nf, fstep)
        assert s.shape == (2, nf, 3, 1024) and s.dtype == torch.int32 and s.device.type == "meta"
    for bad in ((0, 6, 1), (0, 2, 5), (5, 1, 1), (-1, 1, 1), (0, 0, 1), (0, 2, 0)):
        with pytest.raises(RuntimeError):
            t.colour_hist(x, *bad)
    with pytest.raises(RuntimeError):
        t.colour_hist(torch.empty(2, 4, 5, 24, 40, device="meta"), 0, 5, 1)
    with pytest.raises(RuntimeError):
        t.colour_hist(torch.empty(1, 3, 1, 8193, 8192, device="meta"), 0, 1, 1)   # more than 2^26 pixels
    src = torch.empty(2, 5, 3, 1024, dtype=torch.int32, device="meta")
    two = torch.empty(2, 2, 3, 1024, dtype=torch.int32, device="meta")
    for base in (None, torch.empty_like(x)):
        y, tab = t.colour_transfer(x, base, src, two, 551, 0.5)
        assert y.shape == x.shape and y.dtype == torch.float32 and tab.shape == (2, 5, 3, 1024) and tab.dtype == torch.float32
        assert y.device.type == tab.device.type == "meta"
    for bad in ((None, src, two, 0, 0.5), (None, src, two, 2 ** 26 + 1, 0.5), (None, src, two, 551, 1.5), (None, src, two, 551, -0.1),
                (None, src, two, 551, float("nan")), (None, src[:, :4], two, 551, 0.5), (None, src, src, 551, 0.5),
                (None, src[:1], two[:1], 551, 0.5), (None, src.float(), two, 551, 0.5), (None, src, two.long(), 551, 0.5),
                (x[:, :, :4], src, two, 551, 0.5), (x.double(), src, two, 551, 0.5)):
        with pytest.raises(RuntimeError):
            t.colour_transfer(x, *bad)
    with pytest.raises((RuntimeError, NotImplementedError)):                      # no CPU kernel is registered: no fallback
        t.colour_hist(torch.zeros(1, 3, 2, 4, 4), 0, 2, 1)
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.colour_transfer(torch.zeros(1, 3, 2, 4, 4), None, torch.zeros(1, 2, 3, 1024, dtype=torch.int32),
                          torch.zeros(1, 2, 3, 1024, dtype=torch.int32), 16, 1.0)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_colour_hist_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    x = (ctypes.c_float * (2 * 3 * 5 * 24 * 40))()
    hist = (ctypes.c_int32 * (2 * 5 * 3 * 1024 + 1))()
    ws = (ctypes.c_int32 * 4096)()
    one = 3 * 1024 * 4                                                          # bytes of one frame's part

    def params(**kw):
        p = _lib.TcColourHistParams(x=ctypes.addressof(x), b=2, t=5, h=24, w=40, f0=0, nf=5, fstep=1, hist=ctypes.addressof(hist))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rc(**kw):
        return lib.tc_colour_hist(ctypes.byref(params(**kw)), None)

    def need(**kw):
        return lib.tc_colour_hist_workspace(ctypes.byref(params(**kw)))
    assert lib.tc_colour_hist(None, None) == -1 and lib.tc_colour_hist_workspace(None) == 0
    # well formed, no workspace: every one of these passes the argument checks and stops at the workspace
    for ok in ({}, dict(f0=0, nf=2, fstep=4), dict(f0=1, nf=1, fstep=0), dict(f0=4, nf=1, fstep=-3), dict(f0=1, nf=2, fstep=3),
               dict(h=8192, w=8192)):                                             # 2^26 pixels: the largest frame
        assert rc(**ok) == -4, ok
    assert rc(x=None) == -1 and rc(hist=None) == -1
    for name in ("b", "t", "h", "w", "nf"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -2}) == -1, name
    assert rc(f0=-1) == -1 and rc(f0=5, nf=1) == -1                               # a first frame outside the clip
    assert rc(nf=6) == -1 and rc(f0=1) == -1 and rc(nf=2, fstep=5) == -1          # a later frame outside the clip
    assert rc(nf=2, fstep=0) == -1 and rc(nf=2, fstep=-1) == -1
    assert rc(nf=2, fstep=2 ** 31 - 1) == -1                                      # no wrap-around in the last frame's index
    assert rc(hist=ctypes.addressof(hist) + 2) == -2
    assert rc(h=8193, w=8192) == -3 and rc(h=1, w=2 ** 26 + 1) == -3              # more than 2^26 pixels
    assert rc(b=2 ** 26, t=1, nf=1, h=128, w=128) == -3                          # more than 2^31 - 1 blocks
    # the workspace: b * nf * 3 * parts * 1024 int32, parts = min(16, ceil(h * w / 1024))
    assert need() == 2 * 5 * one and need(nf=2, fstep=4) == 2 * 2 * one and need(b=1) == 5 * one
    assert need(h=50, w=83) == 2 * 5 * 5 * one and need(h=320, w=512) == 2 * 5 * 16 * one and need(h=17, w=23) == 2 * 5 * one
    for refused in (dict(x=None), dict(nf=6), dict(hist=ctypes.addressof(hist) + 2), dict(h=0), dict(h=8193, w=8192)):
        assert need(**refused) == 0
    assert rc(workspace=None, workspace_bytes=1 << 30) == -4
    assert rc(workspace=ctypes.addressof(ws), workspace_bytes=2 * 5 * one - 1) == -4
    assert rc(workspace=ctypes.addressof(ws) + 2, workspace_bytes=1 << 30) == -2
    assert not any(hist) and not any(ws)


def test_colour_transfer_refuses_bad_arguments_before_any_launch():
    """every request here has exactly one defect: a well-formed one would launch, and these are host pointers"""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    n = 2 * 3 * 5 * 24 * 40
    x, out, base = (ctypes.c_float * n)(), (ctypes.c_float * (2 * n))(), (ctypes.c_float * (2 * n))()
    src, two = (ctypes.c_int32 * (2 * 5 * 3 * 1024 + 1))(), (ctypes.c_int32 * (2 * 2 * 3 * 1024 + 1))()
    table = (ctypes.c_float * (2 * 5 * 3 * 1024 + 1))()

    def rc(**kw):
        p = _lib.TcColourTransferParams(x=ctypes.addressof(x), base=None, out=ctypes.addressof(out), b=2, t=5, h=24, w=40,
                                        src=ctypes.addressof(src), ref=ctypes.addressof(two), ref_pixels=551, strength=1.0,
                                        table=ctypes.addressof(table))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_colour_transfer(ctypes.byref(p), None)
    assert lib.tc_colour_transfer(None, None) == -1
    for name in ("x", "out", "src", "ref", "table"):
        assert rc(**{name: None}) == -1, name
    for name in ("b", "t", "h", "w"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -3}) == -1, name
    for s in (-0.25, 1.0 + 2.0 ** -20, 2.0, float("inf"), float("-inf"), float("nan")):
        assert rc(strength=s) == -1, s
    assert rc(ref_pixels=0) == -1 and rc(ref_pixels=-551) == -1
    a = ctypes.addressof(out) + 4 * n                                            # the middle of `out`: room on both sides
    for shift in (4, -4, 4 * n - 4, 4 - 4 * n, 16, 4 * 24 * 40):                  # out overlaps x without being x
        assert rc(x=a, out=a + shift) == -1, shift
    c = ctypes.addressof(base) + 4 * n
    for shift in (0, 4, -4, 4 * n - 4, 4 - 4 * n, 16):                            # out overlaps base, or is base
        assert rc(base=c, out=c + shift) == -1, shift
    for name, buf in (("src", src), ("ref", two), ("table", table)):
        assert rc(**{name: ctypes.addressof(buf) + 2}) == -2, name
    # the size limit of the exact integer products (in place: a clip that large claims more bytes than lie between x and out)
    assert rc(h=8193, w=8192, out=ctypes.addressof(x)) == -3 and rc(ref_pixels=2 ** 26 + 1) == -3
    assert not any(out) and not any(table)


def test_both_bindings_refuse_cpu_tensors_wrong_dtypes_and_sizes():
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    x = torch.zeros(2, 3, 5, 8, 8)
    src, two = torch.zeros(2, 5, 3, 1024, dtype=torch.int32), torch.zeros(2, 2, 3, 1024, dtype=torch.int32)
    for be in (HipOps(), TorchLibOps()):
        with pytest.raises(TooncrafterHipError):
            be.colour_hist(x)
        with pytest.raises(TooncrafterHipError):
            be.colour_transfer(x, src, two, 64, 1.0)
        with pytest.raises(TooncrafterHipError):
            be.colour_transfer(x, src, two, 64, 1.0, out=x)


# ---------------------------------------------------------------- the statement on its own

def test_edge_values_fall_into_the_stated_bins():
    assert np.array_equal(ref.bins(ref.EDGE_VALUES), ref.EDGE_BINS)
    one = np.float32(1.0 / 512 - 1)
    assert ref.bins(one) == 1 and ref.bins(np.nextafter(one, np.float32(-2))) == 0
    assert ref.bins(np.float32(-0.0)) == ref.bins(np.float32(0.0)) == 512
    assert ref.bins(np.nextafter(np.float32(1), np.float32(0))) == 1023          # the add rounds to 2
    h = ref.hist(np.tile(ref.EDGE_VALUES, 3).reshape(1, 3, 1, 1, -1))
    assert h.sum() == 3 * len(ref.EDGE_VALUES) and (h[0, 0, :, 0] == 6).all() and (h[0, 0, :, 1023] == 4).all()


def test_exact_consequences_of_the_statement():
    video, ends = ref.toon_frames(3, 1, 3, 7, 9), ref.toon_frames(4, 1, 2, 5, 6)
    # strength 0: clamp(x), or clamp(base)
    assert np.array_equal(ref.transfer(video, ends, 0.0)[0], ref.clamp(video))
    other = ref.toon_frames(5, 1, 3, 7, 9)
    assert np.array_equal(ref.transfer(video, ends, 0.0, base=other)[0], ref.clamp(other))
    for method in ("hm", "hm_mkl_hm"):
        assert np.array_equal(ref.match(video, ends, method, 0.0)["out"], ref.clamp(video))
    # self-match: at every frame index and strength, also against the same histogram at a multiple of the pixel count
    t = 4
    one = np.repeat(ref.toon_frames(6, 2, 1, 7, 9), t, axis=2)
    own = ref.hist(one)
    for mult in (1, 3):
        for strength in (1.0, 0.75, 0.3):
            d, _ = ref.table(own, own[:, :2] * mult, 63, 63 * mult)
            assert not d.any() and not np.signbit(d).any()
            assert np.array_equal(ref.apply(one, d, strength), ref.clamp(one))
    # whole-bin shift: 64 bins = 0.125, nothing clipped
    x = ref.grid_frames(7, 1, 3, 7, 9)
    target = (x[:, :, :1] + np.float32(0.125)).astype(np.float32)
    assert np.array_equal(ref.bins(target), ref.bins(x[:, :, :1]) + 64)
    y, d = ref.transfer(x[:, :, :1], np.concatenate([target, target], axis=2), 1.0)
    assert np.array_equal(y, target) and set(np.unique(d)) == {np.float32(0.0), np.float32(0.125)}
    assert np.array_equal(d != 0, ref.hist(x[:, :, :1]) > 0)
    # monotone over the occupied bins, at every frame
    _, big = ref.table(ref.hist(video), ref.hist(ends), 63, 30)
    for f in range(3):
        for k in range(3):
            tt = big[0, f, k][~np.isnan(big[0, f, k])]
            assert len(tt) > 3 and (np.diff(tt) >= 0).all()


def single_bin(b, t, h, w, value):
    return np.full((b, 3, t, h, w), value, np.float32)


@pytest.mark.parametrize("case", ["empty_bins", "single_bin_reference", "single_bin_source"])
def test_every_entry_brackets_its_rank_in_separate_integer_arithmetic(case):
    """A_{j-1} / m < P_i / 2n <= A_j / m for the bin j - 1 that T lands in (T in (j - 1, j]), at f = 0 against the first reference
    and at f = t - 1 against the last, with python integers and fractions"""
    t, n, m = 3, 7 * 9, 5 * 6
    video = single_bin(1, t, 7, 9, 0.3) if case == "single_bin_source" else ref.toon_frames(11, 1, t, 7, 9)
    ends = single_bin(1, 2, 5, 6, -0.2) if case == "single_bin_reference" else ref.toon_frames(12, 1, 2, 5, 6)
    src, two = ref.hist(video), ref.hist(ends)
    assert (two == 0).sum() > 3 * 2 * 900                                        # the references have empty bins
    _, big = ref.table(src, two, n, m)
    checked = 0
    for f, e in ((0, 0), (t - 1, 1)):
        for k in range(3):
            s, r = [int(v) for v in src[0, f, k]], [int(v) for v in two[0, e, k]]
            for i in range(ref.BINS):
                if s[i] == 0:
                    assert np.isnan(big[0, f, k, i])
                    continue
                p = 2 * sum(s[:i + 1]) - s[i]
                tt = float(big[0, f, k, i])
                j = int(np.ceil(tt))
                assert 1 <= j <= ref.BINS and j - 1 < tt <= j
                assert Fraction(sum(r[:j - 1]), m) < Fraction(p, 2 * n) <= Fraction(sum(r[:j]), m), (f, k, i)
                assert r[j - 1] > 0
                assert tt == (j - 1) + float(Fraction(p * m - sum(r[:j - 1]) * 2 * n, r[j - 1] * 2 * n))   # one division, one add
                checked += 1
    assert checked >= (6 if case == "single_bin_source" else 60)


def test_compound_seeds_keep_bin_crossings_below_one_percent():
    """The compound's last stage sees the MKL stage's result; a difference there within the MKL stage's bound can move a value
    across a bin edge and so change the two table entries either side.  For the seeds of the GPU test: the reference run with
    every MKL coefficient moved by +-2^-22 max(1, |coefficient|) (the device's coefficient tolerance) differs from the
    unperturbed run by more than the bound at no more than 1 % of the pixels of any frame, all of them in `ref.touched`."""
    for seed in COMPOUND_SEEDS:
        video, ends = cm.frames(seed, 2, 5, 24, 40), cm.frames(100 + seed, 2, 2, 19, 29)
        plain = ref.match(video, ends, "hm_mkl_hm", 0.75)
        allowed = ref.touched(plain["mid"], plain["bound"])
        for shift in (2.0 ** -22, -2.0 ** -22):
            moved = ref.match(video, ends, "hm_mkl_hm", 0.75, mkl_shift=shift)
            bad = np.abs(moved["out"].astype(np.float64) - plain["out"]) > plain["bound"]
            share = bad.any(axis=1).reshape(2, 5, -1).mean(axis=-1)
            print(f"seed {seed} shift {shift:+.3g}: worst share of pixels past the bound {share.max():.4f}")
            assert not (bad & ~allowed).any() and share.max() <= 0.01


# ---------------------------------------------------------------- the public interface and its wiring

def test_colour_match_validates_four_methods():
    from tooncrafter_amd.output import ColourMatch
    assert ColourMatch("hm").strength == 1.0 and ColourMatch("hm_mkl_hm", 0.5).method == "hm_mkl_hm"
    assert ColourMatch() == ColourMatch("mkl", 1.0) and ColourMatch("mean_std", 0).strength == 0
    for bad in (("lab", 1.0), ("HM", 1.0), (1, 1.0), (None, 1.0), ("hm", -0.1), ("hm", 1.01), ("hm_mkl_hm", float("nan")), ("hm", True)):
        with pytest.raises(ValueError):
            ColourMatch(*bad)
    with pytest.raises(ValueError) as e:
        ColourMatch("lab")
    for name in ("mkl", "mean_std", "hm", "hm_mkl_hm"):
        assert repr(name) in str(e.value)


class HistSpy(Spy):
    """the recording backend of the linear methods' test, with the two histogram ops"""

    def colour_match(self, x, src, ref, ref_pixels, method, strength, out=None):
        self.calls.append(("colour_match", tuple(x.shape), tuple(src.shape), float(ref.flatten()[0]), ref_pixels, method, strength,
                           None if out is None else out is x))
        return x + 1000.0, torch.zeros(x.shape[0], x.shape[2], 12)

    def colour_hist(self, x, frames=None):
        self.calls.append(("colour_hist", tuple(x.shape), frames, float(x.flatten()[0])))
        return torch.full((x.shape[0], frames[1], 3, 1024), int(x.flatten()[0]), dtype=torch.int32)

    def colour_transfer(self, x, src, ref, ref_pixels, strength, base=None, out=None):
        self.calls.append(("colour_transfer", tuple(x.shape), tuple(src.shape), int(ref.flatten()[0]), ref_pixels, strength,
                           None if base is None else float(base.flatten()[0]), None if out is None else out is x))
        return x + 100.0, torch.zeros(x.shape[0], x.shape[2], 3, 1024)


@pytest.fixture
def stub_pipeline(monkeypatch):
    """Conditions.from_uint8 / sample / decode_spliced replaced: batch i's keyframe pixels are the constant 10 + first segment,
    its decoded clip the constant 1 + first segment, on a (n, 3, 4, 6, 8) clip with keyframes of (5, 7) pixels"""
    from tooncrafter_amd import clip, ops

    class Cond:
        refs = None

        def __init__(self, first, n):
            self.first, self.n = first, n
            self.ends_px = torch.full((n, 3, 2, 5, 7), 10.0 + first)

    def from_uint8(model, first, last, *, size, t, **options):
        return Cond(int(first[0, 0, 0, 0]), len(first))
    monkeypatch.setattr(clip.Conditions, "from_uint8", staticmethod(from_uint8))
    monkeypatch.setattr(clip, "sample", lambda model, cond, plan, latent_shape, pinned=None, variant=0: cond)
    monkeypatch.setattr(clip, "decode_spliced", lambda model, cond, refs: torch.full((cond.n, 3, 4, 6, 8), 1.0 + cond.first))
    spy = HistSpy()
    prev = ops.set_backend(spy)
    yield clip, spy
    ops.set_backend(prev)


def hm_calls(first, n, strength, pixels=35, ends_hw=(5, 7)):
    """what one batch adds in front of its writer under "hm": the clip's histograms, the keyframes', the transfer (x + 100)"""
    return [("colour_hist", (n, 3, 4, 6, 8), (0, 4, 1), 1.0 + first), ("colour_hist", (n, 3, 2, *ends_hw), (0, 2, 1), 10.0 + first),
            ("colour_transfer", (n, 3, 4, 6, 8), (n, 4, 3, 1024), 10 + first, pixels, strength, None, None)]


def compound_calls(first, n, strength, pixels=35, ends_hw=(5, 7)):
    """... and under "hm_mkl_hm": the transfer at strength 1, the MKL match of its result in place at strength 1, the transfer of
    that in place with the decoded clip as the base of the blend; the keyframes' histograms and statistics once"""
    return hm_calls(first, n, 1.0, pixels, ends_hw) + [
        ("colour_stats", (n, 3, 2, *ends_hw), (0, 2, 1), 10.0 + first), ("colour_stats", (n, 3, 4, 6, 8), (0, 4, 1), 101.0 + first),
        ("colour_match", (n, 3, 4, 6, 8), (n, 4, 9), 10.0 + first, pixels, "mkl", 1.0, True),
        ("colour_hist", (n, 3, 4, 6, 8), (0, 4, 1), 1101.0 + first),
        ("colour_transfer", (n, 3, 4, 6, 8), (n, 4, 3, 1024), 10 + first, pixels, strength, 1.0 + first, True)]


@pytest.mark.parametrize("method,calls,shift", [("hm", hm_calls, 100.0), ("hm_mkl_hm", compound_calls, 1200.0)])
def test_the_histogram_methods_make_exactly_these_calls_then_the_writer(stub_pipeline, method, calls, shift):
    from tooncrafter_amd.output import Colour, ColourMatch
    clip, spy = stub_pipeline
    plan = clip.SamplingPlan(steps=2)
    kf = torch.arange(4, dtype=torch.uint8).view(4, 1, 1, 1).expand(4, 8, 8, 3).contiguous()
    m = ColourMatch(method, 0.5)
    clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan, match=m)
    assert spy.calls == calls(0, 1, 0.5) + [("video_to_uint8", (1, 3, 4, 6, 8), 1.0 + shift)]
    spy.calls.clear()
    c = Colour("bt709")
    clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan, out_fmt="i420", out_colour=c, match=m)
    assert spy.calls == calls(0, 1, 0.5) + [("frames_to_yuv", (1, 3, 4, 6, 8), None, "bicubic", "i420", c, (0, 4), 1.0 + shift)]
    spy.calls.clear()
    clip.synthesize_timeline_u8(None, kf, [2, 4, 4, 1, 1], size=(6, 8), plan=plan, match=m)    # segments (0, 1), then (2): once per batch
    assert spy.calls == calls(0, 2, 0.5) + [("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (0, 1), 1.0 + shift),
                                            ("frames_to_u8", (2, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 1.0 + shift)] + \
        calls(2, 1, 0.5) + [("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 3.0 + shift)]


@pytest.mark.parametrize("method,calls,shift", [("hm", hm_calls, 100.0), ("hm_mkl_hm", compound_calls, 1200.0)])
def test_synthesize_and_image_guided_synthesis_match_every_variant(monkeypatch, stub_pipeline, method, calls, shift):
    from tooncrafter_amd.output import ColourMatch
    clip, spy = stub_pipeline

    class Cond:
        refs, first, n = None, 0, 2
        ends_px = torch.full((2, 3, 2, 6, 8), 10.0)
    monkeypatch.setattr(clip.Conditions, "build", staticmethod(lambda *a, **kw: Cond()))
    monkeypatch.setattr(clip, "sample", lambda model, cond, plan, latent_shape, pinned=None, variant=0: cond)
    videos = torch.zeros(2, 3, 4, 6, 8)
    once = calls(0, 2, 0.25, pixels=48, ends_hw=(6, 8))
    out = clip.synthesize(None, videos, [2, 4, 4, 1, 1], plan=clip.SamplingPlan(steps=2), variants=2, match=ColourMatch(method, 0.25))
    assert out.shape == (2, 2, 3, 4, 6, 8) and spy.calls == once * 2 and float(out.flatten()[0]) == 1.0 + shift
    spy.calls.clear()
    out = clip.image_guided_synthesis(None, [""], videos, [2, 4, 4, 1, 1], n_samples=2, ddim_steps=2, interp=True,
                                      match=ColourMatch(method, 0.25))
    assert spy.calls == once * 2 and float(out.flatten()[0]) == 1.0 + shift


def test_mkl_still_records_its_three_calls(stub_pipeline):
    from tooncrafter_amd.output import ColourMatch
    clip, spy = stub_pipeline
    kf = torch.arange(4, dtype=torch.uint8).view(4, 1, 1, 1).expand(4, 8, 8, 3).contiguous()
    for method in ("mkl", "mean_std"):
        spy.calls.clear()
        clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=clip.SamplingPlan(steps=2), match=ColourMatch(method, 0.5))
        assert spy.calls == [("colour_stats", (1, 3, 2, 5, 7), (0, 2, 1), 10.0), ("colour_stats", (1, 3, 4, 6, 8), (0, 4, 1), 1.0),
                             ("colour_match", (1, 3, 4, 6, 8), (1, 4, 9), 10.0, 35, method, 0.5, None),
                             ("video_to_uint8", (1, 3, 4, 6, 8), 1001.0)]


# ---------------------------------------------------------------- compilation

def test_colour_hist_hip_compiles_for_gfx950_without_scratch(tmp_path):
    from tooncrafter_amd import build
    src = os.path.join(build.CSRC, "colour_hist.hip")
    r = subprocess.run([build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "ch.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {k for k in ("colour_hist_kernel", "colour_hist_finish_kernel", "colour_table_kernel", "colour_lut_kernel") if any(k in n for n in names)}
    assert len(kernels) == 4 and len(names) == len(scratch) == 8, names            # hist: two load forms; apply: those, with and without base
    assert scratch == [0] * 8, list(zip(names, scratch))
