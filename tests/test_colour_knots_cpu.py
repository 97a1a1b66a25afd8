"""Colour match through knots and its gain limit, everything that needs no GPU: the declaration, layout and export of the two
entry points (tc_colour_match_knots, tc_colour_transfer_knots), their Meta kernels and refusals (before any launch, so host
pointers do), the numpy statement of tests/colour_knots_ref.py against the old statements and on its own, the inputs of the GPU
tests (the gain-limit case really is one; the conditioning cap), `ColourMatch` validation and the routing of `match_colour` and
`synthesize` on a recording backend."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import colour_hist_ref as ch
import colour_knots_ref as ref
import colour_match_ref as cm
from conftest import ROOT
from test_colour_hist_cpu import HistSpy

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
MATCH_FIELDS = ("x", "out", "b", "t", "h", "w", "src", "ref", "ref_pixels", "method", "strength", "coefs", "nk", "knot", "max_gain")
TRANSFER_FIELDS = ("x", "base", "out", "b", "t", "h", "w", "src", "ref", "ref_pixels", "strength", "table", "nk", "knot")
G = 4.0                                                                          # the gain limit of the GPU tests


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_and_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name, struct in (("tc_colour_match_knots", _lib.TcColourMatchKnotsParams), ("tc_colour_transfer_knots", _lib.TcColourTransferKnotsParams)):
        assert hasattr(lib, name) and _lib.SYMBOLS[name] == (ctypes.c_int, [ctypes.POINTER(struct), ctypes.c_void_p])
    assert _lib.load().tc_abi_version() == 14 and _lib.TC_ABI_VERSION == 14       # additive: the version stays
    with open(HEADER) as f:
        header = f.read()
    assert "int tc_colour_match_knots(const TcColourMatchKnotsParams* p, void* stream);" in header
    assert "int tc_colour_transfer_knots(const TcColourTransferKnotsParams* p, void* stream);" in header
    assert "colour_course.h" in os.listdir(build.CSRC) and any(h.endswith("colour_course.h") for h in build.HEADERS)


def test_ctypes_structs_match_the_compiled_header(tmp_path):
    from tooncrafter_amd import _lib
    m, tr = _lib.TcColourMatchKnotsParams, _lib.TcColourTransferKnotsParams
    assert tuple(f[0] for f in m._fields_) == MATCH_FIELDS and tuple(f[0] for f in tr._fields_) == TRANSFER_FIELDS
    # the old structs are a prefix of the new ones, field for field
    assert m._fields_[:12] == _lib.TcColourMatchParams._fields_ and tr._fields_[:12] == _lib.TcColourTransferParams._fields_
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %d %zu %zu", TC_ABI_VERSION, TC_TEMPORAL_MAX_FRAMES, sizeof(TcColourMatchKnotsParams), sizeof(TcColourTransferKnotsParams));']
    lines += [f'  printf(" %zu", offsetof(TcColourMatchKnotsParams, {f}));' for f in MATCH_FIELDS]
    lines += [f'  printf(" %zu", offsetof(TcColourTransferKnotsParams, {f}));' for f in TRANSFER_FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [14, 64, ctypes.sizeof(m), ctypes.sizeof(tr)] and _lib.TC_TEMPORAL_MAX_FRAMES == 64
    assert got[4:4 + len(MATCH_FIELDS)] == [getattr(m, f).offset for f in MATCH_FIELDS]
    assert got[4 + len(MATCH_FIELDS):] == [getattr(tr, f).offset for f in TRANSFER_FIELDS]


def test_meta_kernels_infer_shapes_and_refuse():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    assert str(t.colour_match_knots.default._schema) == (
        "tooncrafter::colour_match_knots(Tensor x, Tensor src, Tensor ref, int ref_pixels, int method, float strength, int[] knots, "
        "float max_gain) -> (Tensor, Tensor)")
    assert str(t.colour_transfer_knots.default._schema) == (
        "tooncrafter::colour_transfer_knots(Tensor x, Tensor? base, Tensor src, Tensor ref, int ref_pixels, float strength, "
        "int[] knots) -> (Tensor, Tensor)")
    x = torch.empty(2, 3, 5, 24, 40, device="meta")
    src, three = torch.empty(2, 5, 9, dtype=torch.float64, device="meta"), torch.empty(2, 3, 9, dtype=torch.float64, device="meta")
    y, co = t.colour_match_knots(x, src, three, 391, 1, 0.5, [0, 2, 4], 4.0)
    assert y.shape == x.shape and co.shape == (2, 5, 12) and co.dtype == torch.float32 and y.device.type == "meta"
    t.colour_match_knots(x, src, three, 391, 0, 0.5, [1, 2, 3], 0.0)
    for knots, gain in (([0, 4], 4.0), ([0, 2, 2], 4.0), ([0, 4, 2], 4.0), ([0, 2, 5], 4.0), ([-1, 2, 4], 4.0), ([], 4.0),
                        ([0, 2, 4], 0.5), ([0, 2, 4], -1.0), ([0, 2, 4], float("inf")), ([0, 2, 4], float("nan"))):
        with pytest.raises(RuntimeError):
            t.colour_match_knots(x, src, three, 391, 1, 0.5, knots, gain)
    hs, h3 = torch.empty(2, 5, 3, 1024, dtype=torch.int32, device="meta"), torch.empty(2, 3, 3, 1024, dtype=torch.int32, device="meta")
    for base in (None, torch.empty_like(x)):
        y, tab = t.colour_transfer_knots(x, base, hs, h3, 391, 0.5, [0, 2, 4])
        assert y.shape == x.shape and tab.shape == (2, 5, 3, 1024) and tab.dtype == torch.float32
    for knots in ([0, 4], [0, 2, 2], [0, 2, 5], [-1, 2, 4], []):
        with pytest.raises(RuntimeError):
            t.colour_transfer_knots(x, None, hs, h3, 391, 0.5, knots)
    with pytest.raises(RuntimeError):                                              # 65 knots
        t.colour_transfer_knots(torch.empty(1, 3, 70, 8, 8, device="meta"), None, torch.empty(1, 70, 3, 1024, dtype=torch.int32, device="meta"),
                                torch.empty(1, 65, 3, 1024, dtype=torch.int32, device="meta"), 391, 0.5, list(range(65)))
    with pytest.raises((RuntimeError, NotImplementedError)):                      # no CPU kernel is registered: no fallback
        t.colour_match_knots(torch.zeros(1, 3, 2, 4, 4), torch.zeros(1, 2, 9, dtype=torch.float64), torch.zeros(1, 2, 9, dtype=torch.float64),
                             16, 1, 1.0, [0, 1], 0.0)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_the_knots_calls_refuse_bad_arguments_before_any_launch():
    """every request here has exactly one defect: a well-formed one would launch, and these are host pointers"""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    n = 2 * 3 * 5 * 24 * 40
    x, out, base = (ctypes.c_float * n)(), (ctypes.c_float * (2 * n))(), (ctypes.c_float * (2 * n))()
    src, three, coefs = (ctypes.c_double * (2 * 5 * 9 + 1))(), (ctypes.c_double * (2 * 3 * 9 + 1))(), (ctypes.c_float * (2 * 5 * 12))()
    hsrc, h3 = (ctypes.c_int32 * (2 * 5 * 3 * 1024 + 1))(), (ctypes.c_int32 * (2 * 3 * 3 * 1024 + 1))()
    table = (ctypes.c_float * (2 * 5 * 3 * 1024 + 1))()

    def match_rc(knots=(0, 2, 4), **kw):
        p = _lib.TcColourMatchKnotsParams(x=ctypes.addressof(x), out=ctypes.addressof(out), b=2, t=5, h=24, w=40, src=ctypes.addressof(src),
                                          ref=ctypes.addressof(three), ref_pixels=391, method=1, strength=1.0,
                                          coefs=ctypes.addressof(coefs), nk=len(knots), max_gain=4.0)
        p.knot[:len(knots)] = knots
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_colour_match_knots(ctypes.byref(p), None)

    def transfer_rc(knots=(0, 2, 4), **kw):
        p = _lib.TcColourTransferKnotsParams(x=ctypes.addressof(x), base=None, out=ctypes.addressof(out), b=2, t=5, h=24, w=40,
                                             src=ctypes.addressof(hsrc), ref=ctypes.addressof(h3), ref_pixels=391, strength=1.0,
                                             table=ctypes.addressof(table), nk=len(knots))
        p.knot[:len(knots)] = knots
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_colour_transfer_knots(ctypes.byref(p), None)
    assert lib.tc_colour_match_knots(None, None) == -1 and lib.tc_colour_transfer_knots(None, None) == -1
    for rc in (match_rc, transfer_rc):
        # the knots: nk outside [1, 64], not strictly increasing, outside [0, t)
        assert rc(nk=0) == -1 and rc(nk=-1) == -1 and rc(nk=65) == -1
        for knots in ((0, 2, 2), (0, 4, 2), (2, 0, 4), (0, 2, 5), (-1, 2, 4), (5,), (0, 0)):
            assert rc(knots=knots) == -1, knots
        # what the old entry points refuse, with the same codes
        for name in ("x", "out", "src", "ref"):
            assert rc(**{name: None}) == -1, name
        for name in ("b", "t", "h", "w"):
            assert rc(**{name: 0}) == -1 and rc(**{name: -3}) == -1, name
        for s in (-0.25, 1.0 + 2.0 ** -20, 2.0, float("inf"), float("nan")):
            assert rc(strength=s) == -1, s
        assert rc(ref_pixels=0) == -1 and rc(ref_pixels=-391) == -1
        a = ctypes.addressof(out) + 4 * n                                        # the middle of `out`: room on both sides
        for shift in (4, -4, 4 * n - 4, 4 - 4 * n):                               # out overlaps x without being x
            assert rc(x=a, out=a + shift) == -1, shift
    for g in (-1.0, -0.0 - 2.0 ** -20, 0.5, 1.0 - 2.0 ** -20, float("inf"), float("-inf"), float("nan")):
        assert match_rc(max_gain=g) == -1, g
    assert match_rc(method=2) == -1 and match_rc(method=-1) == -1 and match_rc(coefs=None) == -1 and transfer_rc(table=None) == -1
    assert match_rc(src=ctypes.addressof(src) + 4) == -2 and match_rc(ref=ctypes.addressof(three) + 4) == -2
    for name, buf in (("src", hsrc), ("ref", h3), ("table", table)):
        assert transfer_rc(**{name: ctypes.addressof(buf) + 2}) == -2, name
    c = ctypes.addressof(base) + 4 * n
    for shift in (0, 4, -4):                                                      # out overlaps base, or is base
        assert transfer_rc(base=c, out=c + shift) == -1, shift
    assert transfer_rc(h=8193, w=8192, out=ctypes.addressof(x)) == -3 and transfer_rc(ref_pixels=2 ** 26 + 1) == -3
    assert not any(out) and not any(table) and not any(coefs)


def test_the_python_check_of_knots_and_gains():
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    x, src, three = torch.zeros(2, 3, 5, 8, 8), torch.zeros(2, 5, 9, dtype=torch.float64), torch.zeros(2, 3, 9, dtype=torch.float64)
    for be in (HipOps(), TorchLibOps()):                                          # no CPU fallback behind the new keywords either
        with pytest.raises(TooncrafterHipError):
            be.colour_match(x, src, three, 64, "mkl", 1.0, knots=(0, 2, 4), max_gain=4.0)
        with pytest.raises(TooncrafterHipError):
            be.colour_transfer(x, torch.zeros(2, 5, 3, 1024, dtype=torch.int32), torch.zeros(2, 3, 3, 1024, dtype=torch.int32), 64, 1.0,
                               knots=(0, 2, 4))
    for knots in ((0, 2, 2), (0, 5), (-1, 4), (), (1.0, 2.0), (True, 2), tuple(range(65))):
        with pytest.raises(ValueError):
            HipOps._colour_knots(knots, None, 5 if len(knots) < 65 else 70, "colour_match")
    for gain in (0.5, -1.0, float("inf"), float("nan"), True):
        with pytest.raises(ValueError):
            HipOps._colour_knots((0, 4), gain, 5, "colour_match")
    assert HipOps._colour_knots(None, 4, 5, "m") == ((0, 4), 4.0) and HipOps._colour_knots(None, None, 1, "m") == ((0,), 0.0)
    assert HipOps._colour_knots([1, 3], 0, 5, "m") == ((1, 3), 0.0)


# ---------------------------------------------------------------- the statement

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_the_two_ends_without_a_limit_are_the_old_statements_bit_for_bit(shape):
    """coefficients, tables and outputs, all four methods: knots {0, t - 1} ({0} with the first reference when t = 1)"""
    b, t, h, w = shape
    x, ends = cm.frames(sum(shape), b, t, h, w), cm.frames(1 + sum(shape), b, 2, *ref.REF_HW)
    knots, refs = ref.stack_targets(ends, t, None)
    assert knots == ((0, t - 1) if t > 1 else (0,)) and refs.shape[2] == len(knots)
    n, m = h * w, ref.REF_HW[0] * ref.REF_HW[1]
    for method in ("mkl", "mean_std"):
        for strength in (1.0, 0.5):
            old = cm.coefs(cm.frame_stats(x), cm.frame_stats(ends), n, m, method, strength)
            new = ref.coefs(cm.frame_stats(x), cm.frame_stats(refs), knots, n, m, method, strength)
            assert np.array_equal(old.view(np.int64), new.view(np.int64))
            assert np.array_equal(cm.match(x, ends, method, strength)[0], ref.match(x, refs, knots, method, strength)[0])
    toon = ch.toon_frames(sum(shape), b, t, h, w)
    tends = ch.toon_frames(1 + sum(shape), b, 2, *ref.REF_HW)
    _, trefs = ref.stack_targets(tends, t, None)
    old_d, old_t = ch.table(ch.hist(toon), ch.hist(tends), n, m)
    new_d, new_t = ref.table(ch.hist(toon), ch.hist(trefs), knots, n, m)
    assert np.array_equal(old_d.view(np.int32), new_d.view(np.int32)) and np.array_equal(old_t, new_t, equal_nan=True)
    for strength in (1.0, 0.5):
        assert np.array_equal(ch.match(toon, tends, "hm", strength)["out"], ref.transfer(toon, trefs, knots, strength)[0])
    if h * w <= 64:                                                               # the compound once per t, on the small frames
        old = ch.match(toon, tends, "hm_mkl_hm", 0.5)
        new, mid = ref.compound(toon, trefs, knots, 0.5)
        assert np.array_equal(old["out"], new) and np.array_equal(old["mid"], mid)


def test_the_course_picks_the_stated_knots():
    assert [ref.course((0, 4), f) for f in range(5)] == [(0, True, 0.0), (0, False, 0.25), (0, False, 0.5), (0, False, 0.75), (1, True, 0.0)]
    assert [ref.course((1, 3), f) for f in range(5)] == [(0, True, 0.0), (0, True, 0.0), (0, False, 0.5), (1, True, 0.0), (1, True, 0.0)]
    assert [ref.course((2,), f) for f in range(5)] == [(0, True, 0.0)] * 5
    assert [ref.course((0, 2, 4), f) for f in range(5)] == [(0, True, 0.0), (0, False, 0.5), (1, True, 0.0), (1, False, 0.5), (2, True, 0.0)]
    assert [ref.course((0, 3, 4), f)[2] for f in (1, 2)] == [1 / 3, 2 / 3]
    every = tuple(range(64))
    assert all(ref.course(every, f) == (f, True, 0.0) for f in range(64))


def test_a_frame_between_two_knots_with_equal_references_gets_that_reference_exactly():
    """in the table bit for bit (q + w (q - q) = q); in the linear target up to one rounding of (1 - w) m + w m"""
    b, t, h, w = 1, 5, 7, 9
    x = ch.toon_frames(3, b, t, h, w)
    one = ch.toon_frames(4, b, 1, *ref.REF_HW)
    same = np.concatenate([one, one], axis=2)
    d, _ = ref.table(ch.hist(x), ch.hist(same), (1, 3), h * w, 17 * 23)
    alone, _ = ref.table(ch.hist(x), ch.hist(one), (2,), h * w, 17 * 23)
    assert np.array_equal(d.view(np.int32), alone.view(np.int32))
    y = cm.frames(5, b, t, h, w)
    r = cm.frames(6, b, 1, *ref.REF_HW)
    two = ref.coefs(cm.frame_stats(y), cm.frame_stats(np.concatenate([r, r], axis=2)), (1, 3), h * w, 17 * 23, "mean_std", 1.0)
    single = ref.coefs(cm.frame_stats(y), cm.frame_stats(r), (2,), h * w, 17 * 23, "mean_std", 1.0)
    assert np.array_equal(two[:, [0, 1, 3, 4]], single[:, [0, 1, 3, 4]]) and np.abs(two[:, 2] - single[:, 2]).max() <= 2.0 ** -50


@pytest.mark.parametrize("shape", ref.SHAPES[:2], ids=ref.IDS[:2])
def test_tables_are_monotone_over_occupied_bins(shape):
    b, t, h, w = shape
    x = ch.toon_frames(sum(shape), b, t, h, w)
    for knots in ref.KNOT_SETS[t]:
        refs = ch.toon_frames(7 + len(knots), b, len(knots), *ref.REF_HW)
        d, big = ref.table(ch.hist(x), ch.hist(refs), knots, h * w, 17 * 23)
        for row in big.reshape(-1, ch.BINS):
            on = row[~np.isnan(row)]
            assert on.size and (np.diff(on) >= 0).all()
        assert (d[np.isnan(big)] == 0).all()


def test_mean_std_at_gain_one_is_the_identity_and_the_mean_shift():
    b, t, h, w = 2, 5, 7, 9
    x, refs = cm.frames(1, b, t, h, w), cm.frames(2, b, 3, *ref.REF_HW)
    src, three = cm.frame_stats(x), cm.frame_stats(refs)
    for s in (1.0, 0.5):
        co = ref.coefs(src, three, (0, 2, 4), h * w, 17 * 23, "mean_std", s, max_gain=1.0)
        assert np.array_equal(co[..., :9], np.broadcast_to(np.eye(3).reshape(9), co[..., :9].shape))
        for i in range(b):
            moments = [cm.moments(three[i, k], 17 * 23) for k in range(3)]
            for f in range(t):
                assert np.array_equal(co[i, f, 9:], s * (ref.target(moments, (0, 2, 4), f)[0] - cm.moments(src[i, f], h * w)[0]))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_the_gain_limit_case_of_the_gpu_tests_is_one_and_is_well_conditioned(shape):
    """near-flat source frames (spread 0.002 .. 0.005) against references of spread 0.25 .. 0.6: without a limit the largest
    eigenvalue of every frame's map exceeds 4 g = 16 (in the reverse case, "steep", it stays below 1 / (4 g)); with the limit the
    eigenvalues lie in [1 / g, g] and o + A m_s = m_t; and the conditioning cap of the existing tests, cond(C_s + eps I) <= 1e3,
    holds on every clip the GPU tests take coefficients of"""
    b, t, h, w = shape
    n, m = h * w, ref.REF_HW[0] * ref.REF_HW[1]
    for kind in ("random", "flat", "steep"):
        x, refs = ref.inputs(shape, kind)
        src, every = cm.frame_stats(x), cm.frame_stats(refs)
        for i in range(b):
            for f in range(t):
                assert cm.cond(cm.moments(src[i, f], n)[1]) <= 1e3
        if kind == "random":
            continue
        for knots in ref.KNOT_SETS[t]:
            some = every[:, :len(knots)]
            for method in ("mkl", "mean_std"):
                gains = ref.unlimited_gain(src, some, knots, n, m, method)
                assert gains.min() > 4 * G if kind == "flat" else gains.max() < 1 / (4 * G), (kind, knots, method, gains.min(), gains.max())
                co = ref.coefs(src, some, knots, n, m, method, 1.0, max_gain=G)
                a = co[..., :9].reshape(b, t, 3, 3)
                lam = np.linalg.eigvalsh(0.5 * (a + a.transpose(0, 1, 3, 2)))
                assert lam.min() >= (1 / G) * (1 - 2.0 ** -40) and lam.max() <= G * (1 + 2.0 ** -40)
                for i in range(b):
                    moments = [cm.moments(some[i, k], m) for k in range(len(knots))]
                    for f in range(t):
                        ms, mt = cm.moments(src[i, f], n)[0], ref.target(moments, knots, f)[0]
                        assert np.abs(co[i, f, 9:] + a[i, f] @ ms - mt).max() <= 2.0 ** -45


def test_the_limited_map_by_jacobi_and_by_lapack_agree():
    """the figure behind the GPU test of the limited coefficients: the Jacobi statement against the same limited map by
    numpy.linalg.eigh (the pattern of colour_match_ref.mkl_eigh), on the cases of that test, relative to max(1, |value|)"""
    worst = 0.0
    for shape in ref.SHAPES:
        b, t, h, w = shape
        for kind in ("flat", "steep"):
            x, refs = ref.inputs(shape, kind)
            src, every = cm.frame_stats(x), cm.frame_stats(refs)
            for knots in ref.KNOT_SETS[t]:
                for strength in (1.0, 0.5):
                    a = ref.coefs(src, every[:, :len(knots)], knots, h * w, 17 * 23, "mkl", strength, max_gain=G)
                    e = ref.coefs(src, every[:, :len(knots)], knots, h * w, 17 * 23, "mkl", strength, max_gain=G, eig=np.linalg.eigh)
                    worst = max(worst, (np.abs(a - e) / np.maximum(1.0, np.abs(e))).max())
    print(f"limited map, Jacobi against eigh: worst relative gap {worst:.3g} = {worst * 2 ** 22:.3g} x 2^-22")
    assert worst <= 2.0 ** -40                                                    # far inside the 2^-22 of the device test


# ---------------------------------------------------------------- the public interface and its wiring

def test_colour_match_validates_max_gain_and_targets():
    from tooncrafter_amd.output import ColourMatch
    m = ColourMatch()
    assert m.max_gain is None and m.targets == "ends" and m == ColourMatch("mkl", 1.0, None, "ends")
    assert ColourMatch("mkl", max_gain=1).max_gain == 1 and ColourMatch("mean_std", 0.5, 4.0, "pinned").targets == "pinned"
    assert ColourMatch("hm_mkl_hm", max_gain=2.5).max_gain == 2.5 and ColourMatch("hm", targets="pinned").max_gain is None
    for bad in (0, 0.5, 1 - 2.0 ** -30, -4.0, float("inf"), float("nan"), True, "4", [4.0]):
        with pytest.raises(ValueError):
            ColourMatch("mkl", max_gain=bad)
    with pytest.raises(ValueError) as e:
        ColourMatch("hm", max_gain=4.0)
    assert "hm" in str(e.value)
    for bad in ("inner", "Pinned", None, 1, True):
        with pytest.raises(ValueError):
            ColourMatch("mkl", targets=bad)


class KnotSpy(HistSpy):
    """the recording backend of the existing routing tests; the knots keywords are recorded only when they are passed, so a call
    without them records what it always did"""

    def colour_match(self, x, src, ref, ref_pixels, method, strength, out=None, **kw):
        got = super().colour_match(x, src, ref, ref_pixels, method, strength, out=out)
        if kw:
            self.calls[-1] += (tuple(ref.shape), kw)
        return got

    def colour_transfer(self, x, src, ref, ref_pixels, strength, base=None, out=None, **kw):
        got = super().colour_transfer(x, src, ref, ref_pixels, strength, base=base, out=out)
        if kw:
            self.calls[-1] += (tuple(ref.shape), kw)
        return got


@pytest.fixture
def spy():
    from tooncrafter_amd import ops
    s = KnotSpy()
    prev = ops.set_backend(s)
    yield s
    ops.set_backend(prev)


def test_match_colour_without_inner_and_max_gain_makes_exactly_the_old_calls(spy):
    from tooncrafter_amd.output import ColourMatch, match_colour
    video, ends = torch.full((2, 3, 4, 6, 8), 1.0), torch.full((2, 3, 2, 5, 7), 10.0)
    want = {"mkl": [("colour_stats", (2, 3, 2, 5, 7), (0, 2, 1), 10.0), ("colour_stats", (2, 3, 4, 6, 8), (0, 4, 1), 1.0),
                    ("colour_match", (2, 3, 4, 6, 8), (2, 4, 9), 10.0, 35, "mkl", 0.5, None)],
            "hm": [("colour_hist", (2, 3, 4, 6, 8), (0, 4, 1), 1.0), ("colour_hist", (2, 3, 2, 5, 7), (0, 2, 1), 10.0),
                   ("colour_transfer", (2, 3, 4, 6, 8), (2, 4, 3, 1024), 10, 35, 0.5, None, None)]}
    for method in ("mkl", "hm"):
        for inner in (None, {}):
            for targets in ("ends", "pinned"):
                spy.calls.clear()
                match_colour(video, ends, ColourMatch(method, 0.5, targets=targets), inner=inner)
                assert spy.calls == want[method], (method, inner, targets)
        spy.calls.clear()
        match_colour(video, ends, ColourMatch(method, 0.5))                        # the parent's signature
        assert spy.calls == want[method]


def test_match_colour_with_inner_targets_or_a_limit_goes_through_the_knots(spy):
    from tooncrafter_amd.output import ColourMatch, match_colour
    video, ends = torch.full((2, 3, 4, 6, 8), 1.0), torch.full((2, 3, 2, 5, 7), 10.0)
    inner = {2: torch.full((2, 3, 5, 7), 20.0)}
    kn = dict(knots=(0, 2, 3), max_gain=None)
    match_colour(video, ends, ColourMatch("mkl", 0.5), inner=inner)
    assert spy.calls == [("colour_stats", (2, 3, 3, 5, 7), (0, 3, 1), 10.0), ("colour_stats", (2, 3, 4, 6, 8), (0, 4, 1), 1.0),
                         ("colour_match", (2, 3, 4, 6, 8), (2, 4, 9), 10.0, 35, "mkl", 0.5, None, (2, 3, 9), kn)]
    spy.calls.clear()
    match_colour(video, ends, ColourMatch("mean_std", 0.5, max_gain=4.0))          # a limit alone: the two ends as knots
    assert spy.calls == [("colour_stats", (2, 3, 2, 5, 7), (0, 2, 1), 10.0), ("colour_stats", (2, 3, 4, 6, 8), (0, 4, 1), 1.0),
                         ("colour_match", (2, 3, 4, 6, 8), (2, 4, 9), 10.0, 35, "mean_std", 0.5, None, (2, 2, 9), dict(knots=(0, 3), max_gain=4.0))]
    spy.calls.clear()
    match_colour(video, ends, ColourMatch("hm", 0.5), inner=inner)
    assert spy.calls == [("colour_hist", (2, 3, 4, 6, 8), (0, 4, 1), 1.0), ("colour_hist", (2, 3, 3, 5, 7), (0, 3, 1), 10.0),
                         ("colour_transfer", (2, 3, 4, 6, 8), (2, 4, 3, 1024), 10, 35, 0.5, None, None, (2, 3, 3, 1024), dict(knots=(0, 2, 3)))]
    spy.calls.clear()
    match_colour(video, ends, ColourMatch("hm_mkl_hm", 0.5, max_gain=2.0), inner=inner)     # all three stages use the knots
    k3 = dict(knots=(0, 2, 3))
    assert spy.calls == [
        ("colour_hist", (2, 3, 4, 6, 8), (0, 4, 1), 1.0), ("colour_hist", (2, 3, 3, 5, 7), (0, 3, 1), 10.0),
        ("colour_transfer", (2, 3, 4, 6, 8), (2, 4, 3, 1024), 10, 35, 1.0, None, None, (2, 3, 3, 1024), k3),
        ("colour_stats", (2, 3, 3, 5, 7), (0, 3, 1), 10.0), ("colour_stats", (2, 3, 4, 6, 8), (0, 4, 1), 101.0),
        ("colour_match", (2, 3, 4, 6, 8), (2, 4, 9), 10.0, 35, "mkl", 1.0, True, (2, 3, 9), dict(knots=(0, 2, 3), max_gain=2.0)),
        ("colour_hist", (2, 3, 4, 6, 8), (0, 4, 1), 1101.0),
        ("colour_transfer", (2, 3, 4, 6, 8), (2, 4, 3, 1024), 10, 35, 0.5, 1.0, True, (2, 3, 3, 1024), k3)]
    # an inner index on an endpoint replaces that endpoint's image: two knots, the first image the inner one
    spy.calls.clear()
    match_colour(video, ends, ColourMatch("mkl"), inner={0: torch.full((2, 3, 5, 7), 30.0)})
    assert spy.calls[0] == ("colour_stats", (2, 3, 2, 5, 7), (0, 2, 1), 30.0) and spy.calls[2][-1] == dict(knots=(0, 3), max_gain=None)
    for bad in ({4: inner[2]}, {-1: inner[2]}, {2: torch.zeros(2, 3, 6, 8)}, {2: torch.zeros(1, 3, 5, 7)}, {True: inner[2]}, {2: None}):
        with pytest.raises(ValueError):
            match_colour(video, ends, ColourMatch("mkl"), inner=bad)


def test_synthesize_hands_pinned_keyframes_over_only_when_asked(monkeypatch, spy):
    from tooncrafter_amd import clip
    from tooncrafter_amd.output import ColourMatch

    class Cond:
        refs = None
        ends_px = torch.full((2, 3, 2, 6, 8), 10.0)
    monkeypatch.setattr(clip.Conditions, "build", staticmethod(lambda *a, **kw: Cond()))
    monkeypatch.setattr(clip, "pin_frames", lambda model, frames, t: ("x0", "mask"))
    monkeypatch.setattr(clip, "sample", lambda model, cond, plan, latent_shape, pinned=None, variant=0: cond)
    monkeypatch.setattr(clip, "decode_spliced", lambda model, cond, refs: torch.full((2, 3, 4, 6, 8), 1.0))
    videos, px = torch.zeros(2, 3, 4, 6, 8), {2: torch.full((2, 3, 6, 8), 20.0)}
    plan = clip.SamplingPlan(steps=2)
    ends = [("colour_stats", (2, 3, 2, 6, 8), (0, 2, 1), 10.0), ("colour_stats", (2, 3, 4, 6, 8), (0, 4, 1), 1.0),
            ("colour_match", (2, 3, 4, 6, 8), (2, 4, 9), 10.0, 48, "mkl", 1.0, None)]
    clip.synthesize(None, videos, [2, 4, 4, 1, 1], plan=plan, keyframes=px, match=ColourMatch("mkl"))
    assert spy.calls == ends
    spy.calls.clear()
    clip.synthesize(None, videos, [2, 4, 4, 1, 1], plan=plan, match=ColourMatch("mkl", targets="pinned"))     # nothing pinned
    assert spy.calls == ends
    spy.calls.clear()
    clip.synthesize(None, videos, [2, 4, 4, 1, 1], plan=plan, keyframes=px, match=ColourMatch("mkl", targets="pinned"), variants=2)
    assert spy.calls == [("colour_stats", (2, 3, 3, 6, 8), (0, 3, 1), 10.0), ("colour_stats", (2, 3, 4, 6, 8), (0, 4, 1), 1.0),
                         ("colour_match", (2, 3, 4, 6, 8), (2, 4, 9), 10.0, 48, "mkl", 1.0, None, (2, 3, 9),
                          dict(knots=(0, 2, 3), max_gain=None))] * 2
