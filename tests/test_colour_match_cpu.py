"""Colour match of decoded frames to their keyframes, everything that needs no GPU: the declaration, layout and export of the C
ABI (tc_colour_stats, tc_colour_match), the Meta kernels, every refusal (before any launch, so host pointers do), the float64
statement of tests/colour_match_ref.py on its own (Jacobi against LAPACK, the match property, the timeline seam), the wiring
of `match=` through the synthesis calls on a recording backend, and the compile of csrc/colour_match.hip without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import colour_match_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
STATS_FIELDS = ("x", "b", "t", "h", "w", "f0", "nf", "fstep", "stats", "workspace", "workspace_bytes")
MATCH_FIELDS = ("x", "out", "b", "t", "h", "w", "src", "ref", "ref_pixels", "method", "strength", "coefs")
ENTRY_POINTS = ("tc_colour_stats_workspace", "tc_colour_stats", "tc_colour_match")


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_and_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_colour_stats_workspace"] == (ctypes.c_int64, [ctypes.POINTER(_lib.TcColourStatsParams)])
    assert _lib.SYMBOLS["tc_colour_stats"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcColourStatsParams), ctypes.c_void_p])
    assert _lib.SYMBOLS["tc_colour_match"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcColourMatchParams), ctypes.c_void_p])
    assert _lib.load().tc_abi_version() == 14 and _lib.TC_ABI_VERSION == 14       # additive: the version stays
    with open(HEADER) as f:
        header = f.read()
    assert "int64_t tc_colour_stats_workspace(const TcColourStatsParams* p);" in header
    assert "int tc_colour_stats(const TcColourStatsParams* p, void* stream);" in header
    assert "int tc_colour_match(const TcColourMatchParams* p, void* stream);" in header
    assert "colour_match.hip" in build.SOURCES
    for name in ("colour_stats", "colour_match"):
        assert callable(getattr(HipOps, name)) and getattr(TorchLibOps, name) is not getattr(HipOps, name)


def test_ctypes_structs_match_the_compiled_header(tmp_path):
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcColourStatsParams._fields_) == STATS_FIELDS
    assert tuple(f[0] for f in _lib.TcColourMatchParams._fields_) == MATCH_FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %d %d %d %zu %zu", TC_ABI_VERSION, TC_COLOUR_STATS, TC_COLOUR_MEAN_STD, TC_COLOUR_MKL, '
             'sizeof(TcColourStatsParams), sizeof(TcColourMatchParams));']
    lines += [f'  printf(" %zu", offsetof(TcColourStatsParams, {f}));' for f in STATS_FIELDS]
    lines += [f'  printf(" %zu", offsetof(TcColourMatchParams, {f}));' for f in MATCH_FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:6] == [14, 9, 0, 1, ctypes.sizeof(_lib.TcColourStatsParams), ctypes.sizeof(_lib.TcColourMatchParams)]
    assert got[6:6 + len(STATS_FIELDS)] == [getattr(_lib.TcColourStatsParams, f).offset for f in STATS_FIELDS]
    assert got[6 + len(STATS_FIELDS):] == [getattr(_lib.TcColourMatchParams, f).offset for f in MATCH_FIELDS]
    assert (_lib.TC_COLOUR_STATS, _lib.TC_COLOUR_METHODS) == (9, ref.METHODS)


def test_meta_kernels_infer_shapes_and_dtypes():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    assert str(t.colour_stats.default._schema) == "tooncrafter::colour_stats(Tensor x, int f0, int nf, int fstep) -> Tensor"
    assert str(t.colour_match.default._schema) == ("tooncrafter::colour_match(Tensor x, Tensor src, Tensor ref, int ref_pixels, "
                                                   "int method, float strength) -> (Tensor, Tensor)")
    x = torch.empty(2, 3, 5, 24, 40, device="meta")
    for (f0, nf, fstep) in ((0, 5, 1), (0, 2, 4), (1, 1, 1), (4, 1, 0), (1, 2, 3)):
        s = t.colour_stats(x, f0, nf, fstep)
        assert s.shape == (2, nf, 9) and s.dtype == torch.float64 and s.device.type == "meta"
    for bad in ((0, 6, 1), (0, 2, 5), (5, 1, 1), (-1, 1, 1), (0, 0, 1), (0, 2, 0)):
        with pytest.raises(RuntimeError):
            t.colour_stats(x, *bad)
    with pytest.raises(RuntimeError):
        t.colour_stats(torch.empty(2, 4, 5, 24, 40, device="meta"), 0, 5, 1)
    src, two = torch.empty(2, 5, 9, dtype=torch.float64, device="meta"), torch.empty(2, 2, 9, dtype=torch.float64, device="meta")
    for method in (0, 1):
        y, co = t.colour_match(x, src, two, 77, method, 0.5)
        assert y.shape == x.shape and y.dtype == torch.float32 and co.shape == (2, 5, 12) and co.dtype == torch.float32
        assert y.device.type == co.device.type == "meta"
    for bad in ((src, two, 77, 2, 0.5), (src, two, 77, -1, 0.5), (src, two, 0, 1, 0.5), (src, two, 77, 1, 1.5), (src, two, 77, 1, -0.1),
                (src, two, 77, 1, float("nan")), (src[:, :4], two, 77, 1, 0.5), (src, src, 77, 1, 0.5), (src[:1], two[:1], 77, 1, 0.5)):
        with pytest.raises(RuntimeError):
            t.colour_match(x, *bad)
    with pytest.raises((RuntimeError, NotImplementedError)):                      # no CPU kernel is registered: no fallback
        t.colour_stats(torch.zeros(1, 3, 2, 4, 4), 0, 2, 1)
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.colour_match(torch.zeros(1, 3, 2, 4, 4), torch.zeros(1, 2, 9, dtype=torch.float64), torch.zeros(1, 2, 9, dtype=torch.float64),
                       16, 1, 1.0)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_colour_stats_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    x = (ctypes.c_float * (2 * 3 * 5 * 24 * 40))()
    stats = (ctypes.c_double * (2 * 5 * 9))()
    ws = (ctypes.c_double * 4096)()

    def params(**kw):
        p = _lib.TcColourStatsParams(x=ctypes.addressof(x), b=2, t=5, h=24, w=40, f0=0, nf=5, fstep=1, stats=ctypes.addressof(stats))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rc(**kw):
        return lib.tc_colour_stats(ctypes.byref(params(**kw)), None)

    def need(**kw):
        return lib.tc_colour_stats_workspace(ctypes.byref(params(**kw)))
    assert lib.tc_colour_stats(None, None) == -1 and lib.tc_colour_stats_workspace(None) == 0
    # well formed, no workspace: every one of these passes the argument checks and stops at the workspace
    for ok in ({}, dict(f0=0, nf=2, fstep=4), dict(f0=1, nf=1, fstep=0), dict(f0=4, nf=1, fstep=-3), dict(f0=1, nf=2, fstep=3)):
        assert rc(**ok) == -4, ok
    assert rc(x=None) == -1 and rc(stats=None) == -1
    for name in ("b", "t", "h", "w", "nf"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -2}) == -1, name
    assert rc(f0=-1) == -1 and rc(f0=5, nf=1) == -1                               # a first frame outside the clip
    assert rc(nf=6) == -1 and rc(f0=1) == -1 and rc(nf=2, fstep=5) == -1          # a later frame outside the clip
    assert rc(nf=2, fstep=0) == -1 and rc(nf=2, fstep=-1) == -1
    assert rc(nf=2, fstep=2 ** 31 - 1) == -1                                      # no wrap-around in the last frame's index
    assert rc(stats=ctypes.addressof(stats) + 4) == -2
    # the workspace: b * nf * parts * 9 doubles, parts = min(64, ceil(h * w / 2048)), a function of h * w alone
    assert need() == 2 * 5 * 1 * 72 and need(nf=2, fstep=4) == 2 * 2 * 72 and need(b=1) == 5 * 72
    assert need(h=128, w=160, t=5) == 2 * 5 * 10 * 72 and need(h=320, w=512) == 2 * 5 * 64 * 72 and need(h=64, w=33) == 2 * 5 * 2 * 72
    for refused in (dict(x=None), dict(nf=6), dict(stats=ctypes.addressof(stats) + 4), dict(h=0)):
        assert need(**refused) == 0
    assert rc(workspace=None, workspace_bytes=1 << 30) == -4
    assert rc(workspace=ctypes.addressof(ws), workspace_bytes=2 * 5 * 72 - 1) == -4
    assert rc(workspace=ctypes.addressof(ws) + 4, workspace_bytes=1 << 30) == -2
    assert not any(stats) and not any(ws)


def test_colour_match_refuses_bad_arguments_before_any_launch():
    """every request here has exactly one defect: a well-formed one would launch, and these are host pointers"""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    n = 2 * 3 * 5 * 24 * 40
    x, out = (ctypes.c_float * n)(), (ctypes.c_float * (2 * n))()
    src, two, coefs = (ctypes.c_double * (2 * 5 * 9 + 1))(), (ctypes.c_double * (2 * 2 * 9 + 1))(), (ctypes.c_float * (2 * 5 * 12))()

    def rc(**kw):
        p = _lib.TcColourMatchParams(x=ctypes.addressof(x), out=ctypes.addressof(out), b=2, t=5, h=24, w=40, src=ctypes.addressof(src),
                                     ref=ctypes.addressof(two), ref_pixels=960, method=1, strength=1.0, coefs=ctypes.addressof(coefs))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_colour_match(ctypes.byref(p), None)
    assert lib.tc_colour_match(None, None) == -1
    for name in ("x", "out", "src", "ref", "coefs"):
        assert rc(**{name: None}) == -1, name
    for name in ("b", "t", "h", "w"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -3}) == -1, name
    assert rc(method=2) == -1 and rc(method=-1) == -1
    for s in (-0.25, 1.0 + 2.0 ** -20, 2.0, float("inf"), float("-inf"), float("nan")):
        assert rc(strength=s) == -1, s
    assert rc(ref_pixels=0) == -1 and rc(ref_pixels=-960) == -1
    a = ctypes.addressof(out) + 4 * n                                            # the middle of `out`: room on both sides
    for shift in (4, -4, 4 * n - 4, 4 - 4 * n, 16, 4 * 24 * 40):                  # out overlaps x without being x
        assert rc(x=a, out=a + shift) == -1, shift
    assert rc(src=ctypes.addressof(src) + 4) == -2 and rc(ref=ctypes.addressof(two) + 4) == -2
    assert not any(out) and not any(coefs)


def test_both_bindings_refuse_cpu_tensors_wrong_dtypes_and_strides():
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    x = torch.zeros(2, 3, 5, 8, 8)
    src, two = torch.zeros(2, 5, 9, dtype=torch.float64), torch.zeros(2, 2, 9, dtype=torch.float64)
    for be in (HipOps(), TorchLibOps()):
        with pytest.raises(TooncrafterHipError):
            be.colour_stats(x)
        with pytest.raises(TooncrafterHipError):
            be.colour_match(x, src, two, 64, "mkl", 1.0)
        with pytest.raises(TooncrafterHipError):
            be.colour_match(x, src, two, 64, "mkl", 1.0, out=x)
    # the frames of a statistics request are checked on the host, by one function for both bindings
    hip = HipOps()
    for bad in (dict(frames=(0, 6, 1)), dict(frames=(5, 1, 1)), dict(frames=(0, 2, 0)), dict(frames=(-1, 1, 1)), dict(frames=(0, 0, 1))):
        with pytest.raises(ValueError):
            hip._colour_frames(bad["frames"], 5, "colour_stats")
    assert hip._colour_frames(None, 5, "s") == (0, 5, 1) and hip._colour_frames((4, 1, 0), 5, "s") == (4, 1, 0)


# ---------------------------------------------------------------- the statement on its own

def test_jacobi_mkl_equals_the_lapack_statement():
    """200 random pairs of 960-pixel frames: the eight-sweep Jacobi map against numpy.linalg.eigh's, both float64.  1e-8 is the
    level at which an fp32 coefficient could first change (measured on these pairs: 1.1e-11 worst, cond(S) up to 1.4e3)."""
    rng = np.random.default_rng(5)
    worst, worst_cond = 0.0, 0.0
    for case in range(200):
        spread = (0.25, 0.6) if case % 2 else (10.0 ** rng.uniform(-3.5, -2.0), 0.45)        # every second pair badly conditioned
        x = ref.frames(1000 + case, 1, 2, 24, 40, spread=spread)
        st = ref.frame_stats(x)[0]
        (_, cs), (_, ct) = ref.moments(st[0], 960), ref.moments(st[1], 960)
        worst = max(worst, float(np.abs(ref.mkl(cs, ct) - ref.mkl_eigh(cs, ct)).max()))
        worst_cond = max(worst_cond, float(ref.cond(cs)))
        lam, v = ref.jacobi(cs)
        assert np.allclose(np.sort(lam), np.linalg.eigvalsh(cs), rtol=0, atol=1e-15) and np.allclose(v @ v.T, np.eye(3), atol=1e-14)
    print(f"worst |jacobi - eigh| = {worst:.3g} at condition numbers up to {worst_cond:.3g}")
    assert worst <= 1e-8 and worst_cond > 1e3


@pytest.mark.parametrize("method", ["mkl", "mean_std"])
def test_matched_frame_has_the_targets_moments(method):
    """strength 1: (m, C) of the matched frame (not clamped) equal the target's within eps (1 + |A|_2^2) + 1e-12, which follows
    from A (S - eps I) A = T - eps A^2; mean_std matches the diagonal only."""
    for seed in range(12):
        t = 1 + seed % 4
        video, ends = ref.frames(seed, 1, t, 24, 40), ref.frames(100 + seed, 1, 2, 17, 23)
        src, two = ref.frame_stats(video), ref.frame_stats(ends)
        y, co = ref.match(video, ends, method, 1.0)
        (m0, c0), (m1, c1) = ref.moments(two[0, 0], 17 * 23), ref.moments(two[0, 1], 17 * 23)
        for f in range(t):
            ms, cs = ref.moments(src[0, f], 960)
            assert ref.cond(cs) <= 1e3
            mt, ct = ref.target(m0, c0, m1, c1, f, t)
            a = co[0, f, :9].reshape(3, 3)
            bound = ref.EPS * (1.0 + np.linalg.norm(a, 2) ** 2) + 1e-12
            my, cy = ref.plain_moments(y[0, :, f])
            assert np.abs(my - mt).max() <= bound
            err = np.abs(cy - ct)
            assert (err.max() if method == "mkl" else np.diag(err).max()) <= bound, (seed, f, err.max(), bound)
        if t > 1:                                                                 # the ends of the course are the keyframes
            assert np.array_equal(ref.target(m0, c0, m1, c1, 0, t)[1], c0) and np.array_equal(ref.target(m0, c0, m1, c1, t - 1, t)[1], c1)


def test_exact_consequences_of_the_statement():
    video, ends = ref.frames(3, 1, 3, 7, 9), ref.frames(4, 1, 2, 7, 9)
    for method in ("mkl", "mean_std"):
        _, co = ref.match(video, ends, method, 0.0)
        assert np.array_equal(co.astype(np.float32), np.broadcast_to(np.r_[np.eye(3).reshape(9), np.zeros(3)], co.shape))
    one = video[:, :, :1]
    _, co = ref.match(one, np.concatenate([one, one], axis=2), "mean_std", 1.0)   # a frame against its own statistics
    assert np.array_equal(co, np.r_[np.eye(3).reshape(9), np.zeros(3)].reshape(1, 1, 12))


def test_timeline_seam_has_one_target():
    """two segments that share a keyframe: the last frame of the first and frame 0 of the second have the same target, to the
    bit, and it is the shared keyframe's own (m, C)"""
    kf = ref.frames(9, 1, 3, 12, 20)                                              # three keyframes as three frames
    st = ref.frame_stats(kf)[0]
    (m0, c0), (m1, c1), (m2, c2) = (ref.moments(s, 240) for s in st)
    for t in (2, 4, 16):
        ma, ca = ref.target(m0, c0, m1, c1, t - 1, t)
        mb, cb = ref.target(m1, c1, m2, c2, 0, t)
        assert np.array_equal(ma, mb) and np.array_equal(ca, cb) and np.array_equal(ma, m1) and np.array_equal(ca, c1)
    # ... so the two frames, matched, agree in their moments within the property's bound, however they differed before
    a, b = ref.frames(10, 1, 4, 12, 20), ref.frames(11, 1, 4, 12, 20)
    ya, coa = ref.match(a, kf[:, :, 0:2], "mkl", 1.0)
    yb, cob = ref.match(b, kf[:, :, 1:3], "mkl", 1.0)
    (mya, cya), (myb, cyb) = ref.plain_moments(ya[0, :, 3]), ref.plain_moments(yb[0, :, 0])
    bound = sum(ref.EPS * (1.0 + np.linalg.norm(co[:9].reshape(3, 3), 2) ** 2) + 1e-12 for co in (coa[0, 3], cob[0, 0]))
    assert np.abs(mya - myb).max() <= bound and np.abs(cya - cyb).max() <= bound
    before = np.abs(ref.plain_moments(ref.clamp(a[0, :, 3]))[0] - ref.plain_moments(ref.clamp(b[0, :, 0]))[0]).max()
    assert before > 100 * bound                                                   # the case says something


# ---------------------------------------------------------------- the public interface and its wiring

def test_colour_match_validates():
    from tooncrafter_amd.output import ColourMatch
    assert ColourMatch() == ColourMatch("mkl", 1.0) and ColourMatch("mean_std", 0).strength == 0
    for bad in (("lab", 1.0), ("MKL", 1.0), (1, 1.0), (None, 1.0), ("mkl", -0.1), ("mkl", 1.01), ("mkl", float("nan")),
                ("mkl", "1"), ("mkl", None), ("mkl", True)):
        with pytest.raises(ValueError):
            ColourMatch(*bad)
    with pytest.raises(Exception):
        ColourMatch().strength = 0.5                                              # frozen


def test_conditions_keep_their_positional_form_and_carry_the_keyframes():
    from tooncrafter_amd import clip
    c = clip.Conditions({}, None, None, None, torch.zeros(1), None, False)        # the seven fields there were
    assert c.ends_px is None and c.three_way is False
    assert [f for f in clip.Conditions.__dataclass_fields__][-1] == "ends_px"

    class Inner:
        conditioning_key = "crossattn"

    class Model:
        device, model = "cpu", Inner()
        get_learned_conditioning = staticmethod(lambda prompts: torch.zeros(len(prompts), 2, 4))
        image_proj_model = staticmethod(lambda tokens: tokens)
        embedder = staticmethod(lambda image: torch.zeros(image.shape[0], 1, 4))
    videos = torch.arange(2 * 3 * 4 * 2 * 2, dtype=torch.float32).view(2, 3, 4, 2, 2)
    held = clip.Conditions.build(Model(), videos, fs=3, guided=False)
    assert held.ends_px.shape == (2, 3, 2, 2, 2) and held.ends_px.is_contiguous()
    assert torch.equal(held.ends_px[:, :, 0], videos[:, :, 0]) and torch.equal(held.ends_px[:, :, 1], videos[:, :, 3])
    free = clip.Conditions.build(Model(), videos, fs=3, guided=False, hold_endpoints=False)
    assert torch.equal(free.ends_px[:, :, 0], videos[:, :, 0]) and torch.equal(free.ends_px[:, :, 1], videos[:, :, 0])


class Spy:
    """a recording backend: the colour ops and the writers, nothing else"""

    def __init__(self):
        self.calls = []

    def colour_stats(self, x, frames=None):
        self.calls.append(("colour_stats", tuple(x.shape), frames, float(x.flatten()[0])))
        return torch.full((x.shape[0], frames[1], 9), float(x.flatten()[0]), dtype=torch.float64)

    def colour_match(self, x, src, ref, ref_pixels, method, strength, out=None):
        self.calls.append(("colour_match", tuple(x.shape), tuple(src.shape), float(ref.flatten()[0]), ref_pixels, method, strength, out))
        return x + 1000.0, torch.zeros(x.shape[0], x.shape[2], 12)

    def video_to_uint8(self, video):
        self.calls.append(("video_to_uint8", tuple(video.shape), float(video.flatten()[0])))
        return torch.zeros(1)

    def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
        self.calls.append(("frames_to_u8", tuple(x.shape), size, filter, fmt, frames, float(x.flatten()[0])))
        return torch.zeros(1)

    def frames_to_yuv(self, x, size=None, filter="bicubic", fmt="nv12", colour=None, frames=None, out=None, strides=None):
        self.calls.append(("frames_to_yuv", tuple(x.shape), size, filter, fmt, colour, frames, float(x.flatten()[0])))
        return torch.zeros(1)


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
    spy = Spy()
    prev = ops.set_backend(spy)
    yield clip, spy
    ops.set_backend(prev)


def test_match_none_makes_the_calls_there_were_and_no_colour_op(stub_pipeline):
    from tooncrafter_amd.output import Colour
    clip, spy = stub_pipeline
    plan = clip.SamplingPlan(steps=2)
    kf = torch.arange(4, dtype=torch.uint8).view(4, 1, 1, 1).expand(4, 8, 8, 3).contiguous()
    c = Colour("bt709")
    clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan)
    clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan, match=None)
    clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan, out_size=(12, 16), out_fmt="nv12", out_colour=c,
                       match=None)
    assert spy.calls == [("video_to_uint8", (1, 3, 4, 6, 8), 1.0)] * 2 + [("frames_to_yuv", (1, 3, 4, 6, 8), (12, 16), "bicubic", "nv12", c, (0, 4), 1.0)]
    for kw in ({}, dict(match=None)):
        spy.calls.clear()
        clip.synthesize_timeline_u8(None, kf, [2, 4, 4, 1, 1], size=(6, 8), plan=plan, **kw)
        assert spy.calls == [("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (0, 1), 1.0),
                             ("frames_to_u8", (2, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 1.0),
                             ("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 3.0)], kw
    import inspect
    for fn in (clip.synthesize, clip.synthesize_u8, clip.synthesize_timeline_u8, clip.image_guided_synthesis):
        assert inspect.signature(fn).parameters["match"].default is None, fn.__name__


def test_a_colour_match_runs_stats_stats_match_then_the_writer(stub_pipeline):
    from tooncrafter_amd.output import Colour, ColourMatch
    clip, spy = stub_pipeline
    plan = clip.SamplingPlan(steps=2)
    kf = torch.arange(4, dtype=torch.uint8).view(4, 1, 1, 1).expand(4, 8, 8, 3).contiguous()
    m = ColourMatch("mean_std", 0.5)

    def colour_calls(first, n):
        """what one batch adds in front of its writer: the keyframes' statistics, the clip's, the match (whose result is x + 1000)"""
        return [("colour_stats", (n, 3, 2, 5, 7), (0, 2, 1), 10.0 + first), ("colour_stats", (n, 3, 4, 6, 8), (0, 4, 1), 1.0 + first),
                ("colour_match", (n, 3, 4, 6, 8), (n, 4, 9), 10.0 + first, 35, "mean_std", 0.5, None)]
    clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan, match=m)
    assert spy.calls == colour_calls(0, 1) + [("video_to_uint8", (1, 3, 4, 6, 8), 1001.0)]
    spy.calls.clear()
    c = Colour("bt709")
    clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan, out_fmt="i420", out_colour=c, match=m)
    assert spy.calls == colour_calls(0, 1) + [("frames_to_yuv", (1, 3, 4, 6, 8), None, "bicubic", "i420", c, (0, 4), 1001.0)]
    spy.calls.clear()
    clip.synthesize_timeline_u8(None, kf, [2, 4, 4, 1, 1], size=(6, 8), plan=plan, match=m)    # segments (0, 1), then (2): once per batch
    assert spy.calls == colour_calls(0, 2) + [("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (0, 1), 1001.0),
                                              ("frames_to_u8", (2, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 1001.0)] + \
        colour_calls(2, 1) + [("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 1003.0)]
    for bad in ("mkl", 1.0, ("mkl", 1.0)):
        with pytest.raises(ValueError):
            clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, 4, 1, 1], size=(6, 8), plan=plan, match=bad)


def test_synthesize_matches_every_variant(monkeypatch, stub_pipeline):
    from tooncrafter_amd.output import ColourMatch
    clip, spy = stub_pipeline

    class Cond:
        refs, first, n = None, 0, 2
        ends_px = torch.full((2, 3, 2, 6, 8), 7.0)
    monkeypatch.setattr(clip.Conditions, "build", staticmethod(lambda *a, **kw: Cond()))
    monkeypatch.setattr(clip, "sample", lambda model, cond, plan, latent_shape, pinned=None, variant=0: cond)
    videos = torch.zeros(2, 3, 4, 6, 8)
    out = clip.synthesize(None, videos, [2, 4, 4, 1, 1], plan=clip.SamplingPlan(steps=2), variants=2)
    assert out.shape == (2, 2, 3, 4, 6, 8) and spy.calls == [] and float(out.flatten()[0]) == 1.0
    out = clip.image_guided_synthesis(None, [""], videos, [2, 4, 4, 1, 1], n_samples=2, ddim_steps=2, interp=True, match=ColourMatch())
    assert [c[0] for c in spy.calls] == ["colour_stats", "colour_stats", "colour_match"] * 2
    assert spy.calls[2][3:7] == (7.0, 48, "mkl", 1.0) and float(out.flatten()[0]) == 1001.0


# ---------------------------------------------------------------- compilation

def test_colour_match_hip_compiles_for_gfx950_without_scratch(tmp_path):
    from tooncrafter_amd import build
    src = os.path.join(build.CSRC, "colour_match.hip")
    r = subprocess.run([build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "cm.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {k for k in ("colour_stats_kernel", "colour_finish_kernel", "colour_coefs_kernel", "colour_apply_kernel") if any(k in n for n in names)}
    assert len(kernels) == 4 and len(names) == len(scratch) == 6, names             # stats and apply: a 16-byte and a 4-byte form
    assert scratch == [0] * 6, list(zip(names, scratch))
