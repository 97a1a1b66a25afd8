"""Still regions, everything that needs no GPU: the declaration, layout and export of the C ABI (tc_still_map,
tc_still_composite), their refusals (before any launch, so host pointers do), the numpy statement of tests/still_ref.py against a
brute-force definition (the distance by exhaustive search over cells, the upsampling in Fractions), `StillRegions`, `still_pins`,
`join_pins`, the wiring of `still=` through the three synthesis calls on a recording backend, and the compile of csrc/still.hip
without scratch."""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import still_ref as ref
from conftest import ROOT
from test_colour_match_cpu import Spy

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
MAP_FIELDS = ("ends", "b", "h", "w", "tau", "grow", "feather", "mask", "alpha", "dist")
COMPOSITE_FIELDS = ("video", "ends", "alpha", "out", "b", "t", "h", "w", "f0", "nf")


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_and_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ("tc_still_map", "tc_still_composite"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_still_map"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcStillMapParams), ctypes.c_void_p])
    assert _lib.SYMBOLS["tc_still_composite"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcStillCompositeParams), ctypes.c_void_p])
    assert _lib.load().tc_abi_version() == 14 and _lib.TC_ABI_VERSION == 14       # additive: the version stays
    with open(HEADER) as f:
        header = f.read()
    assert "int tc_still_map(const TcStillMapParams* p, void* stream);" in header
    assert "int tc_still_composite(const TcStillCompositeParams* p, void* stream);" in header
    assert "#define TC_STILL_CELL 8" in header and "#define TC_STILL_MAX_DIST 32" in header
    assert "still.hip" in build.SOURCES
    for name in ("still_map", "still_composite"):                                  # served by the inherited ctypes methods
        assert callable(getattr(HipOps, name)) and getattr(TorchLibOps, name) is getattr(HipOps, name)


def test_ctypes_structs_match_the_compiled_header(tmp_path):
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcStillMapParams._fields_) == MAP_FIELDS
    assert tuple(f[0] for f in _lib.TcStillCompositeParams._fields_) == COMPOSITE_FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %d %d %zu %zu", TC_ABI_VERSION, TC_STILL_CELL, TC_STILL_MAX_DIST, sizeof(TcStillMapParams), '
             'sizeof(TcStillCompositeParams));']
    lines += [f'  printf(" %zu", offsetof(TcStillMapParams, {f}));' for f in MAP_FIELDS]
    lines += [f'  printf(" %zu", offsetof(TcStillCompositeParams, {f}));' for f in COMPOSITE_FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:5] == [14, 8, 32, ctypes.sizeof(_lib.TcStillMapParams), ctypes.sizeof(_lib.TcStillCompositeParams)]
    assert got[5:5 + len(MAP_FIELDS)] == [getattr(_lib.TcStillMapParams, f).offset for f in MAP_FIELDS]
    assert got[5 + len(MAP_FIELDS):] == [getattr(_lib.TcStillCompositeParams, f).offset for f in COMPOSITE_FIELDS]
    assert (_lib.TC_STILL_CELL, _lib.TC_STILL_MAX_DIST) == (8, 32) == (ref.CELL, ref.MAX_DIST)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_still_map_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    b, hh, ww = 2, 16, 24
    ends = (ctypes.c_float * (b * 6 * hh * ww + 8))()
    mask = (ctypes.c_float * (b * 6 + 4))()
    alpha = (ctypes.c_float * (b * hh * ww + 8))()
    dist = (ctypes.c_uint8 * (b * 6 + 4))()
    E, M, A, D = ((ctypes.addressof(v) + 15) & ~15 for v in (ends, mask, alpha, dist))

    def rc(**kw):
        p = _lib.TcStillMapParams(ends=E, b=b, h=hh, w=ww, tau=8, grow=1, feather=2, mask=M, alpha=A, dist=D)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_still_map(ctypes.byref(p), None)
    assert lib.tc_still_map(None, None) == -1
    for name in ("ends", "mask", "alpha", "dist"):
        assert rc(**{name: None}) == -1, name
    for name in ("b", "h", "w"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -8}) == -1, name
    assert rc(tau=-1) == -1 and rc(tau=256) == -1 and rc(grow=-1) == -1 and rc(feather=0) == -1 and rc(feather=-1) == -1
    assert rc(grow=29, feather=3) == -1 and rc(grow=0, feather=32) == -1 and rc(grow=2 ** 31 - 1, feather=2 ** 31 - 1) == -1   # D > 32
    for bad in (dict(h=15), dict(h=17), dict(w=20), dict(w=25), dict(h=4, w=4), dict(h=1), dict(w=7)):
        assert rc(**bad) == -3, bad                                               # not a multiple of 8: the shape error
    assert rc(h=1024, w=1032) == -3 and rc(h=8 * 16385, w=8) == -3                # more than 16384 cells
    assert rc(b=65536) == -3
    assert rc(ends=E + 4) == -2 and rc(alpha=A + 8) == -2 and rc(mask=M + 2) == -2
    assert not any(mask) and not any(alpha) and not any(dist)


def test_still_composite_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    b, t, hh, ww = 1, 3, 8, 16
    n = b * 3 * t * hh * ww
    arena = (ctypes.c_float * (4 * n + 64))()
    base = (ctypes.addressof(arena) + 15) & ~15
    V, O, E, A = base, base + 4 * n, base + 8 * n, base + 8 * n + 4 * b * 6 * hh * ww
    assert A + 4 * b * hh * ww <= ctypes.addressof(arena) + ctypes.sizeof(arena)

    def rc(**kw):
        p = _lib.TcStillCompositeParams(video=V, ends=E, alpha=A, out=O, b=b, t=t, h=hh, w=ww, f0=0, nf=t)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_still_composite(ctypes.byref(p), None)
    assert lib.tc_still_composite(None, None) == -1
    for name in ("video", "ends", "alpha", "out"):
        assert rc(**{name: None}) == -1, name
    for name in ("b", "t", "h", "w"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -1}) == -1, name
    for bad in (dict(nf=0), dict(f0=-1), dict(f0=3, nf=1), dict(f0=1, nf=3), dict(f0=0, nf=4), dict(nf=-1)):
        assert rc(**bad) == -1, bad
    assert rc(h=12) == -3 and rc(w=20) == -3 and rc(t=1, nf=1) == -3 and rc(t=65, nf=1) == -3 and rc(b=65536) == -3
    for name, at in (("video", V), ("ends", E), ("alpha", A), ("out", O)):
        assert rc(**{name: at + 4}) == -2, name
    # out overlapping an input, other than out == video exactly
    assert rc(out=V + 16) == -1 and rc(out=V + 4 * n - 16) == -1 and rc(video=O + 16) == -1
    assert rc(out=E) == -1 and rc(out=A) == -1 and rc(out=E - 4 * n + 16) == -1 and rc(out=A - 16) == -1
    assert not any(arena)


def test_the_binding_refuses_cpu_tensors_wrong_dtypes_and_arguments():
    from tooncrafter_amd import clip, output
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    ends, video, alpha = torch.zeros(1, 3, 2, 16, 24), torch.zeros(1, 3, 4, 16, 24), torch.zeros(1, 16, 24)
    for be in (HipOps(), TorchLibOps()):
        with pytest.raises(TooncrafterHipError):
            be.still_map(ends)
        with pytest.raises(TooncrafterHipError):
            be.still_composite(video, ends, alpha)
        for bad in (dict(tau=-1), dict(tau=256), dict(tau=8.0), dict(tau=True), dict(grow=-1), dict(feather=0), dict(grow=30, feather=2)):
            with pytest.raises(ValueError):
                be.still_map(ends, **bad)
    for bad in (None, ends[0], ends[:, :2], [ends]):
        with pytest.raises(ValueError):
            clip.still_map(bad)
    with pytest.raises(ValueError):
        clip.still_map(ends, rule=8)
    for bad in ((video, ends[:, :, :, :8], alpha), (video, ends, alpha[:, :8]), (video, None, alpha), (video, ends, None)):
        with pytest.raises(ValueError):
            output.hold_still(*bad)


# ---------------------------------------------------------------- the statement against a brute-force definition

def brute_distance(moved, cap):
    h, w = moved.shape
    at = [(i, j) for i in range(h) for j in range(w) if moved[i, j]]
    return np.array([[min([cap] + [max(abs(i - y), abs(j - x)) for y, x in at]) for j in range(w)] for i in range(h)])


def brute_alpha_n(a):
    """the bilinear upsampling of cell values with centres at 8 i + 3.5, in Fractions, times 256"""
    h, w = a.shape

    def axis(p, n):
        u = Fraction(2 * p - 7, 16)                                                # (p - 3.5) / 8: the position in cell units
        i0 = u.numerator // u.denominator
        f = u - i0
        return min(max(i0, 0), n - 1), min(max(i0 + 1, 0), n - 1), 1 - f, f
    out = np.empty((8 * h, 8 * w), dtype=object)
    for y in range(8 * h):
        y0, y1, fy0, fy1 = axis(y, h)
        for x in range(8 * w):
            x0, x1, fx0, fx1 = axis(x, w)
            out[y, x] = 256 * (fy0 * (fx0 * int(a[y0, x0]) + fx1 * int(a[y0, x1])) + fy1 * (fx0 * int(a[y1, x0]) + fx1 * int(a[y1, x1])))
    return out


@pytest.mark.parametrize("h,w,grow,feather,density", [(2, 3, 1, 2, 0.2), (3, 5, 0, 1, 0.1), (5, 4, 2, 3, 0.05), (6, 7, 1, 1, 0.03),
                                                      (4, 4, 0, 3, 0.0), (3, 3, 1, 2, 1.0), (1, 6, 0, 2, 0.2), (7, 1, 3, 28, 0.2)])
def test_the_statement_equals_the_brute_force_definition(h, w, grow, feather, density):
    rng = np.random.default_rng(h * 100 + w * 10 + grow)
    cap = grow + feather + 1
    for trial in range(3):
        moved = rng.random((h, w)) < density
        ends = np.zeros((1, 3, 2, 8 * h, 8 * w), dtype=np.float32)
        for i, j in zip(*np.nonzero(moved)):                                       # one pixel of the cell, in one channel
            ends[0, rng.integers(3), 1, 8 * i + rng.integers(8), 8 * j + rng.integers(8)] = 0.5
        mask, alpha, dist = ref.still_map(ends, 8, grow, feather)
        assert mask.shape == (1, 1, 1, h, w) and alpha.shape == (1, 8 * h, 8 * w) and dist.shape == (1, h, w)
        assert mask.dtype == alpha.dtype == np.float32 and dist.dtype == np.uint8
        assert np.array_equal(ref.moved_cells(ends, 8)[0], moved)
        want = brute_distance(moved, cap)
        assert np.array_equal(dist[0], want)
        assert np.array_equal(mask[0, 0, 0], (want > grow).astype(np.float32))
        a = np.clip(want - grow - 1, 0, feather)
        n = brute_alpha_n(a)
        assert all(v.denominator == 1 for v in n.flat)                             # odd sixteenths per axis: whole 256ths
        n = np.array([[int(v) for v in row] for row in n])
        assert np.array_equal(ref.upsample_n(a[None])[0], n)
        assert np.array_equal(alpha[0], n.astype(np.float32) / np.float32(256 * feather))
        for got, exact in zip(alpha[0].flat, n.flat):                              # one correctly rounded division
            exact = Fraction(int(exact), 256 * feather)
            assert abs(Fraction(float(got)) - exact) * 2 <= Fraction(float(np.spacing(np.float32(got)))), (got, exact)
        assert (alpha[0] == 1.0).sum() == (n == 256 * feather).sum() and (alpha[0] == 0.0).sum() == (n == 0).sum()


def test_exact_consequences_of_the_statement():
    ends = np.random.default_rng(1).uniform(-1, 1, (2, 3, 1, 16, 24)).astype(np.float32).repeat(2, axis=2)
    mask, alpha, dist = ref.still_map(ends, 0, 1, 2)                               # equal keyframes: all still, even at tau 0
    assert (dist == 4).all() and (mask == 1).all() and (alpha == 1).all()
    ends[1, :, 1] += 1.0
    mask, alpha, dist = ref.still_map(ends, 8, 1, 2)                               # clip 1 all moved; clip 0 does not see it
    assert (dist[0] == 4).all() and (alpha[0] == 1).all() and not dist[1].any() and not mask[1].any() and not alpha[1].any()
    thr = np.float32(8) / np.float32(127.5)
    for value, moved in ((thr, False), (np.nextafter(thr, np.float32(1)), True), (np.float32("nan"), True), (np.float32(-0.0), False)):
        e = np.zeros((1, 3, 2, 8, 8), dtype=np.float32)
        e[0, 1, 0, 3, 3] = value
        assert bool(ref.moved_cells(e, 8)[0, 0, 0]) == moved, value
    e = np.zeros((1, 3, 2, 8, 16), dtype=np.float32)
    e[0, 0, :, 0, 0] = (1.5, 3.0)                                                  # beyond the range on one side: clamp to equal
    e[0, 0, :, 0, 1] = (-2.0, -1.0)
    e[0, 0, :, 0, 2] = (np.inf, 1.0)
    e[0, 0, :, 0, 8] = (1.5, -1.5)                                                 # on both sides: 2 apart
    assert ref.moved_cells(e, 8)[0, 0].tolist() == [False, True] and ref.moved_cells(e, 255)[0, 0].tolist() == [False, False]
    e[0, 0, :, 0, 3] = (np.nan, np.nan)                                            # a NaN differs even from itself, at any tau
    assert ref.moved_cells(e, 255)[0, 0].tolist() == [True, False]
    # the composite: alpha 0 keeps v's bits over NaN keyframes, alpha 1 gives key, frames outside the range stay
    rng = np.random.default_rng(2)
    video = rng.uniform(-1, 1, (1, 3, 3, 8, 8)).astype(np.float32)
    ends = rng.uniform(-1, 1, (1, 3, 2, 8, 8)).astype(np.float32)
    alpha = np.zeros((1, 8, 8), dtype=np.float32)
    alpha[0, :, 4:] = 1.0
    alpha[0, 0, 0] = 0.25
    ends[0, :, :, 1, 1] = np.nan
    out = ref.composite(video, ends, alpha, 1, 2)
    assert np.array_equal(out[:, :, 0], video[:, :, 0]) and np.array_equal(out[..., 1:, :4], video[..., 1:, :4]) and not np.isnan(out).any()
    assert np.array_equal(out[0, :, 1, :, 4:], (ends[0, :, 0] + np.float32(0.5) * (ends[0, :, 1] - ends[0, :, 0]))[..., 4:])
    assert np.array_equal(out[0, :, 2, :, 4:], (ends[0, :, 0] + (ends[0, :, 1] - ends[0, :, 0]))[..., 4:])
    key = ends[0, :, 0, 0, 0] + np.float32(0.5) * (ends[0, :, 1, 0, 0] - ends[0, :, 0, 0, 0])
    assert np.array_equal(out[0, :, 1, 0, 0], video[0, :, 1, 0, 0] + np.float32(0.25) * (key - video[0, :, 1, 0, 0]))


# ---------------------------------------------------------------- StillRegions, still_pins, join_pins

def test_still_regions_is_validated_like_a_shot_rule():
    from tooncrafter_amd import clip
    rule = clip.StillRegions()
    assert (rule.tau, rule.grow, rule.feather, rule.pin, rule.composite) == (8, 1, 2, True, True)
    assert clip.StillRegions(tau=0, grow=0, feather=1, pin=False, composite=False).feather == 1
    assert clip.StillRegions(tau=255, grow=28, feather=3).grow == 28               # D = 32
    for bad in (dict(tau=-1), dict(tau=256), dict(tau=1.5), dict(tau=True), dict(tau="8"), dict(grow=-1), dict(grow=1.0), dict(feather=0),
                dict(feather=2.0), dict(grow=29, feather=3), dict(feather=32), dict(pin=1), dict(composite=None), dict(pin="yes")):
        with pytest.raises(ValueError):
            clip.StillRegions(**bad)
    with pytest.raises(Exception):
        rule.tau = 3                                                               # frozen


class FakeCond:
    refs = None

    def __init__(self, n, t, first=0, hw=(16, 24)):
        self.n, self.first = n, first
        self.ends_px = torch.zeros(n, 3, 2, *hw)
        self.ends_px[0, 1, 1, 0, 0] = 0.5                                          # clip 0: cell (0, 0) has moved
        gen = torch.Generator().manual_seed(10 + first)
        self.endpoints = torch.zeros(n, 4, t, hw[0] // 8, hw[1] // 8)
        self.endpoints[:, :, 0] = torch.randn(n, 4, hw[0] // 8, hw[1] // 8, generator=gen)
        self.endpoints[:, :, t - 1] = torch.randn(n, 4, hw[0] // 8, hw[1] // 8, generator=gen)


def interpolated(cond, t):
    z0, z1 = cond.endpoints[:, :, 0], cond.endpoints[:, :, t - 1]
    return torch.stack([z0 + float(np.float32(j) / np.float32(t - 1)) * (z1 - z0) for j in range(t)], dim=2)


def test_still_pins_interpolates_the_endpoint_latents_and_broadcasts_the_mask():
    from tooncrafter_amd import clip
    for t in (2, 4, 16):
        cond = FakeCond(2, t)
        mask = (torch.rand(2, 1, 1, 2, 3) > 0.5).float()
        x0, m = clip.still_pins(cond, mask, t)
        assert x0.shape == (2, 4, t, 2, 3) and x0.dtype == torch.float32 and torch.equal(x0, interpolated(cond, t))
        assert torch.equal(x0[:, :, 0], cond.endpoints[:, :, 0])
        assert m.shape == (2, 1, t, 2, 3) and m.is_contiguous() and all(torch.equal(m[:, :, j], mask[:, :, 0]) for j in range(t))
    cond = FakeCond(2, 4)
    for bad_mask in (mask[:1], mask[:, :, 0], mask.expand(2, 1, 4, 2, 3), None):
        with pytest.raises(ValueError):
            clip.still_pins(cond, bad_mask, 4)
    with pytest.raises(ValueError):
        clip.still_pins(cond, mask, 3)
    cond.endpoints = None
    with pytest.raises(ValueError):
        clip.still_pins(cond, mask, 4)


def test_join_pins_takes_the_maximum_and_a_pinned_frames_own_x0():
    from tooncrafter_amd import clip
    gen = torch.Generator().manual_seed(3)
    xf, xr = torch.randn(2, 4, 4, 2, 3, generator=gen), torch.randn(2, 4, 4, 2, 3, generator=gen)
    mf = torch.tensor([0.0, 0.0, 1.0, 0.0]).view(1, 1, 4, 1, 1).expand(2, 1, 4, 1, 1)
    mr = (torch.rand(2, 1, 1, 2, 3, generator=gen) > 0.5).float().expand(2, 1, 4, 2, 3).contiguous()
    x0, mask = clip.join_pins((xf, mf), (xr, mr))
    assert torch.equal(mask, torch.maximum(mf.expand(2, 1, 4, 2, 3), mr)) and (mask[:, :, 2] == 1).all()
    assert torch.equal(x0[:, :, 2], xf[:, :, 2]) and torch.equal(x0[:, :, [0, 1, 3]], xr[:, :, [0, 1, 3]])
    assert clip.join_pins(None, (xr, mr)) == (xr, mr) and clip.join_pins((xf, mf), None) == (xf, mf) and clip.join_pins(None, None) is None


# ---------------------------------------------------------------- the wiring of still= on a recording backend

class StillSpy(Spy):
    """the recording backend plus the two still ops, computed by the numpy statement"""

    def still_map(self, ends, tau=8, grow=1, feather=2):
        self.calls.append(("still_map", tuple(ends.shape), tau, grow, feather, float(ends.sum())))
        return tuple(torch.from_numpy(v) for v in ref.still_map(ends.numpy(), tau, grow, feather))

    def still_composite(self, video, ends, alpha, frames=None, out=None):
        self.calls.append(("still_composite", tuple(video.shape), float(video.flatten()[0]), frames, out is video))
        return torch.from_numpy(ref.composite(video.numpy(), ends.numpy(), alpha.numpy()))


T = 4
RULE = dict(grow=0, feather=1)                                                     # on the 2 x 3 cells of FakeCond: column 2 is held in full


@pytest.fixture
def stub_pipeline(monkeypatch):
    """Conditions.build / from_uint8, pin_frames, sample and decode_spliced replaced: a batch's conditions are FakeCond(n, T, first
    segment), its decoded clip the constant 1 + first segment on (n, 3, T, 16, 24); every sample call is recorded with its `pinned`"""
    from tooncrafter_amd import clip, ops
    sampled = []

    def from_uint8(model, first, last, *, size, t, **options):
        return FakeCond(len(first), t, int(first[0, 0, 0, 0]))

    def build(model, videos, **options):
        return FakeCond(videos.shape[0], videos.shape[2])

    def pin_frames(model, frames, t):
        x0, mask = torch.zeros(1, 4, t, 2, 3), torch.zeros(1, 1, t, 1, 1)
        for i, px in frames.items():
            x0[:, :, i], mask[:, :, i] = 7.0 + i, 1.0
        return x0, mask

    def sample(model, cond, plan, latent_shape, pinned=None, **kw):
        sampled.append((cond, pinned, kw))
        return cond

    def decode(model, cond, refs):
        return torch.full((cond.n, 3, T, 16, 24), 1.0 + cond.first)
    monkeypatch.setattr(clip.Conditions, "from_uint8", staticmethod(from_uint8))
    monkeypatch.setattr(clip.Conditions, "build", staticmethod(build))
    monkeypatch.setattr(clip, "pin_frames", pin_frames)
    monkeypatch.setattr(clip, "sample", sample)
    monkeypatch.setattr(clip, "decode_spliced", decode)
    spy = StillSpy()
    prev = ops.set_backend(spy)
    yield clip, spy, sampled
    ops.set_backend(prev)


def keyframes_u8(k):
    return torch.arange(k, dtype=torch.uint8).view(k, 1, 1, 1).expand(k, 8, 8, 3).contiguous()


def expected_still(cond, rule):
    mask, alpha, _ = ref.still_map(cond.ends_px.numpy(), rule.tau, rule.grow, rule.feather)
    return torch.from_numpy(mask), torch.from_numpy(alpha)


def test_without_still_the_calls_are_the_calls_there_were(stub_pipeline):
    clip, spy, sampled = stub_pipeline
    plan = clip.SamplingPlan(steps=2)
    kf = keyframes_u8(4)
    for kw in ({}, dict(still=None)):
        spy.calls.clear()
        sampled.clear()
        clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, T, 2, 3], size=(16, 24), plan=plan, **kw)
        assert spy.calls == [("video_to_uint8", (1, 3, T, 16, 24), 1.0)] and sampled[0][1] is None
        spy.calls.clear()
        clip.synthesize_timeline_u8(None, kf, [2, 4, T, 2, 3], size=(16, 24), plan=plan, **kw)
        assert spy.calls == [("frames_to_u8", (1, 3, T, 16, 24), None, "bicubic", "rgb24", (0, 1), 1.0),
                             ("frames_to_u8", (2, 3, T, 16, 24), None, "bicubic", "rgb24", (1, 3), 1.0),
                             ("frames_to_u8", (1, 3, T, 16, 24), None, "bicubic", "rgb24", (1, 3), 3.0)], kw
        spy.calls.clear()
        video = clip.synthesize(None, torch.zeros(1, 3, T, 16, 24), [1, 4, T, 2, 3], plan=plan, variants=2, **kw)
        assert spy.calls == [] and video.shape == (1, 2, 3, T, 16, 24) and (video == 1.0).all()
        assert all(pinned is None for _, pinned, _ in sampled)
    import inspect
    for fn in (clip.synthesize, clip.synthesize_u8, clip.synthesize_timeline_u8):
        assert inspect.signature(fn).parameters["still"].default is None, fn.__name__


def test_the_sampler_receives_the_still_mask_and_the_interpolated_x0(stub_pipeline):
    clip, spy, sampled = stub_pipeline
    rule = clip.StillRegions(**RULE)
    video = clip.synthesize(None, torch.zeros(1, 3, T, 16, 24), [1, 4, T, 2, 3], plan=clip.SamplingPlan(steps=2), variants=2, still=rule)
    assert [c[0] for c in spy.calls] == ["still_map", "still_composite", "still_composite"]       # one map for all variants
    assert spy.calls[0][1:5] == ((1, 3, 2, 16, 24), 8, 0, 1)
    cond = sampled[0][0]
    mask, alpha = expected_still(cond, rule)
    assert mask[0, 0, 0].tolist() == [[0, 1, 1], [1, 1, 1]]
    for k, (_, pinned, kw) in enumerate(sampled):
        assert kw == dict(variant=k)
        assert torch.equal(pinned[0], interpolated(cond, T)) and torch.equal(pinned[1], mask.expand(1, 1, T, 2, 3))
    want = ref.composite(np.ones((1, 3, T, 16, 24), np.float32), cond.ends_px.numpy(), alpha.numpy())
    assert torch.equal(video[:, 0], torch.from_numpy(want)) and torch.equal(video[:, 1], video[:, 0])
    assert (video[0, 0, :, :, :, 20:] == 0).all() and (video[0, 0, :, :, :4, :4] == 1).all()       # the keyframes' zeros | the clip's ones


def test_a_pinned_frame_keeps_its_own_x0_and_the_masks_combine_by_maximum(stub_pipeline):
    clip, spy, sampled = stub_pipeline
    rule = clip.StillRegions(**RULE)
    clip.synthesize(None, torch.zeros(1, 3, T, 16, 24), [1, 4, T, 2, 3], plan=clip.SamplingPlan(steps=2), still=rule,
                    keyframes={2: torch.zeros(1, 3, 16, 24)})
    cond, (x0, mask), _ = sampled[0]
    still_mask, _ = expected_still(cond, rule)
    frames = torch.tensor([0.0, 0.0, 1.0, 0.0]).view(1, 1, T, 1, 1)
    assert torch.equal(mask, torch.maximum(frames.expand(1, 1, T, 2, 3), still_mask.expand(1, 1, T, 2, 3)))
    assert (mask[:, :, 2] == 1).all() and mask[0, 0, 1, 0, 0] == 0
    want = interpolated(cond, T)
    want[:, :, 2] = 9.0                                                            # pin_frames' own x0 of frame 2
    assert torch.equal(x0, want)


def test_pin_and_composite_are_separate_switches(stub_pipeline):
    clip, spy, sampled = stub_pipeline
    plan, kf = clip.SamplingPlan(steps=2), keyframes_u8(2)
    clip.synthesize_u8(None, kf[:1], kf[1:], [1, 4, T, 2, 3], size=(16, 24), plan=plan, still=clip.StillRegions(pin=False, **RULE))
    assert [c[0] for c in spy.calls] == ["still_map", "still_composite", "video_to_uint8"] and sampled[-1][1] is None
    spy.calls.clear()
    clip.synthesize_u8(None, kf[:1], kf[1:], [1, 4, T, 2, 3], size=(16, 24), plan=plan, still=clip.StillRegions(composite=False, **RULE))
    assert [c[0] for c in spy.calls] == ["still_map", "video_to_uint8"] and sampled[-1][1] is not None
    spy.calls.clear()
    clip.synthesize_u8(None, kf[:1], kf[1:], [1, 4, T, 2, 3], size=(16, 24), plan=plan,
                       still=clip.StillRegions(pin=False, composite=False, **RULE))
    assert [c[0] for c in spy.calls] == ["video_to_uint8"] and sampled[-1][1] is None


def test_the_order_is_match_then_composite_then_writer(stub_pipeline):
    from tooncrafter_amd.output import ColourMatch
    clip, spy, sampled = stub_pipeline
    kf = keyframes_u8(2)
    clip.synthesize_u8(None, kf[:1], kf[1:], [1, 4, T, 2, 3], size=(16, 24), plan=clip.SamplingPlan(steps=2), still=clip.StillRegions(**RULE),
                       match=ColourMatch("mkl", 0.5))
    assert [c[0] for c in spy.calls] == ["still_map", "colour_stats", "colour_stats", "colour_match", "still_composite", "video_to_uint8"]
    assert spy.calls[4] == ("still_composite", (1, 3, T, 16, 24), 1001.0, None, True)             # the matched clip, in place
    assert spy.calls[5] == ("video_to_uint8", (1, 3, T, 16, 24), 1001.0)                          # pixel (0, 0) has moved: the clip's
    assert torch.equal(sampled[0][1][0], interpolated(sampled[0][0], T))


def test_a_timeline_maps_every_batch_from_its_own_keyframes_and_leaves_cuts_and_holds_alone(stub_pipeline):
    clip, spy, sampled = stub_pipeline
    rule, plan = clip.StillRegions(**RULE), clip.SamplingPlan(steps=2)
    clip.synthesize_timeline_u8(None, keyframes_u8(4), [2, 4, T, 2, 3], size=(16, 24), plan=plan, still=rule)
    assert [c[0] for c in spy.calls] == ["still_map", "still_composite", "frames_to_u8", "frames_to_u8", "still_map", "still_composite",
                                         "frames_to_u8"]
    assert spy.calls[0][1] == (2, 3, 2, 16, 24) and spy.calls[4][1] == (1, 3, 2, 16, 24)
    assert [(c.first, c.n) for c, _, _ in sampled] == [(0, 2), (2, 1)]
    for cond, pinned, _ in sampled:
        mask, _ = expected_still(cond, rule)
        assert torch.equal(pinned[0], interpolated(cond, T)) and torch.equal(pinned[1], mask.expand(cond.n, 1, T, 2, 3))
    assert (sampled[0][1][1][1] == 1).all() and not (sampled[0][1][1][0] == 1).all()              # clip 1 of the batch is all still
    for held in (spy.calls, sampled):
        held.clear()

    def front(images, size, slots, *, b, t, out=None):
        spy.calls.append(("frames_from_u8",))
        return torch.zeros(b, 3, t, *size)
    spy.frames_from_u8 = front
    clip.synthesize_timeline_u8(None, keyframes_u8(4), [2, 4, T, 2, 3], size=(16, 24), plan=plan, still=rule,
                                shots=clip.ShotPlan(("cut", "tween", "hold")))
    assert [c[0] for c in spy.calls].count("still_map") == 1 and [c[0] for c in spy.calls].count("still_composite") == 1
    assert [(c.first, c.n) for c, _, _ in sampled] == [(1, 1)]


def test_bad_still_arguments_raise_before_anything_is_launched(stub_pipeline):
    clip, spy, sampled = stub_pipeline
    plan, kf, rule = clip.SamplingPlan(steps=2), keyframes_u8(3), clip.StillRegions()
    for bad in ("still", 8, True, dict(tau=8), (8, 1, 2)):
        with pytest.raises(ValueError):
            clip.synthesize(None, torch.zeros(1, 3, T, 16, 24), [1, 4, T, 2, 3], plan=plan, still=bad)
        with pytest.raises(ValueError):
            clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, T, 2, 3], size=(16, 24), plan=plan, still=bad)
        with pytest.raises(ValueError):
            clip.synthesize_timeline_u8(None, kf, [2, 4, T, 2, 3], size=(16, 24), plan=plan, still=bad)
    with pytest.raises(ValueError, match="hold_endpoints"):
        clip.synthesize(None, torch.zeros(1, 3, T, 16, 24), [1, 4, T, 2, 3], plan=plan, still=rule, hold_endpoints=False)
    with pytest.raises(ValueError, match="hold_endpoints"):
        clip.synthesize_u8(None, kf[:1], kf[1:2], [1, 4, T, 2, 3], size=(16, 24), plan=plan, still=rule, hold_endpoints=False)
    assert not spy.calls and not sampled


# ---------------------------------------------------------------- compilation

def test_still_hip_compiles_for_gfx950_without_scratch(tmp_path):
    from tooncrafter_amd import build
    src = os.path.join(build.CSRC, "still.hip")
    r = subprocess.run([build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "still.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {k for k in ("still_scan_kernel", "still_dist_kernel", "still_alpha_kernel", "still_composite_kernel") if any(k in n for n in names)}
    assert len(kernels) == 4 and len(names) == len(scratch) == 5, names            # the composite in place and out of place
    assert scratch == [0] * 5, list(zip(names, scratch))
