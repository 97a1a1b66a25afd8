"""The planar-YUV front end and the keyframe timeline without a GPU: the host matrix builder against the table, the integer
statement (tests/pixel_yuv_ref.py) against an independent one in double, the round trip through the back end's integer rule,
declaration / layout / export, every refusal of tc_frames_from_yuv (all before any device call), the Meta operator, the
Python interface's own checks and the splice arithmetic of synthesize_timeline_u8 on a stub model."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pixel_back_ref as back
import pixel_yuv_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
YUV_FIELDS = ("y", "c0", "c1", "image_stride_y", "image_stride_c", "pitch_y", "pitch_c", "format", "siting", "m", "n", "sh", "sw",
              "slots", "out", "b", "t", "h", "w", "h_bounds", "h_coefs", "h_kmax", "v_bounds", "v_coefs", "v_kmax", "workspace",
              "workspace_bytes")
CASES = [(s, r) for s in ("bt601", "bt709") for r in ("limited", "full")]


# ---------------------------------------------------------------- tc_yuv_matrix

def c_matrix(lib, standard, range_, bits):
    m = (ctypes.c_int32 * 7)(*([-7] * 7))
    rc = lib.tc_yuv_matrix(standard, range_, bits, m)
    return rc, list(m)


def test_yuv_matrix_equals_the_table():
    from tooncrafter_amd import _lib
    from tooncrafter_amd.ops import HipOps
    lib, hip = _lib.load(), HipOps()
    assert len(ref.TABLE) == 8
    for (standard, range_, bits), want in ref.TABLE.items():
        q = 2 ** (bits - 8)
        full = list(want) + [16 * q if range_ == "limited" else 0, 128 * q]
        rc, got = c_matrix(lib, _lib.TC_YUV_STANDARDS[standard], _lib.TC_YUV_RANGES[range_], bits)
        assert rc == 0 and got == full, (standard, range_, bits, got)
        assert ref.matrix(standard, range_, bits) == full                         # the statement's rule gives the table too
        assert hip.yuv_matrix(standard, range_, bits) == full


def test_yuv_matrix_refuses_bad_arguments():
    from tooncrafter_amd import _lib
    from tooncrafter_amd.ops import HipOps
    lib = _lib.load()
    for bad in ((2, 0, 8), (-1, 0, 8), (0, 2, 8), (0, -1, 8), (0, 0, 9), (0, 0, 12), (0, 0, 0), (1, 1, 16)):
        rc, m = c_matrix(lib, *bad)
        assert rc == -1 and m == [-7] * 7, bad                                    # refused, nothing written
    assert lib.tc_yuv_matrix(0, 0, 8, None) == -1
    for bad in (("bt2020", "limited", 8), ("bt601", "studio", 8)):
        with pytest.raises(ValueError):
            HipOps().yuv_matrix(*bad)
    with pytest.raises(_lib.TooncrafterHipError):
        HipOps().yuv_matrix("bt601", "limited", 12)


# ---------------------------------------------------------------- the integer statement against the double statement

def worst_and_count(y, cb, cr, standard, range_, bits):
    a = ref.to_rgb(y, cb, cr, ref.matrix(standard, range_, bits)).astype(np.int16)
    b = ref.to_rgb_double(y, cb, cr, standard, range_, bits).astype(np.int16)
    d = np.abs(a - b)
    return int(d.max()), int(np.count_nonzero(d))


def test_integer_conversion_is_within_one_code_value_of_the_double_matrix_8bit():
    """All 2^24 (Y, Cb, Cr) triples of BT.601 limited, a stride-3 grid of the other three matrices."""
    v = np.arange(256, dtype=np.int64)
    worst = differ = 0
    for y0 in range(0, 256, 16):                                                  # 16 luma values x 65536 chroma pairs at a time
        y, cb, cr = (a.ravel() for a in np.meshgrid(v[y0:y0 + 16], v, v, indexing="ij"))
        w, n = worst_and_count(y, cb, cr, "bt601", "limited", 8)
        worst, differ = max(worst, w), differ + n
    print(f"bt601 limited 8 bit: {differ} of {3 * 256 ** 3} channel values differ, worst {worst}")
    assert worst <= 1
    g = v[::3]
    y, cb, cr = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    for standard, range_ in CASES[1:]:
        w, n = worst_and_count(y, cb, cr, standard, range_, 8)
        print(f"{standard} {range_} 8 bit, stride-3 grid: {n} of {3 * y.size} differ, worst {w}")
        assert w <= 1, (standard, range_)


def test_integer_conversion_is_within_one_code_value_of_the_double_matrix_10bit():
    """A seeded sample of 10^6 10-bit triples per matrix."""
    for k, (standard, range_) in enumerate(CASES):
        y, cb, cr = np.random.default_rng(7100 + k).integers(0, 1024, (3, 10 ** 6))
        w, n = worst_and_count(y, cb, cr, standard, range_, 10)
        print(f"{standard} {range_} 10 bit: {n} of {3 * y.size} differ, worst {w}")
        assert w <= 1, (standard, range_)


def test_round_trip_with_the_back_end_rule():
    """2 x 2 blocks of one colour through the back end's integer rule (tests/pixel_back_ref.py; BT.601 limited, chroma from
    the block's sums) and back with NEAREST: over all 256^3 colours the error is at most (1, 1, 2) in (R, G, B)."""
    m = ref.matrix("bt601", "limited", 8)
    v = np.arange(256, dtype=np.uint8)
    worst = np.zeros(3, np.int64)
    for r0 in range(0, 256, 8):
        colours = np.stack([a.ravel() for a in np.meshgrid(v[r0:r0 + 8], v, v, indexing="ij")], axis=-1)       # (N, 3)
        blocks = np.broadcast_to(colours[:, None, None, :], (len(colours), 2, 2, 3))
        y, cb, cr = back.yuv420(blocks)                                          # (N, 2, 2), (N, 1, 1), (N, 1, 1)
        assert (y == y[:, :1, :1]).all() and ref.upsample(cb, 2, 2, "nearest").shape == y.shape      # four equal pixels: one is converted
        rgb = ref.to_rgb(y[:, 0, 0], cb[:, 0, 0], cr[:, 0, 0], m)
        err = np.abs(rgb.astype(np.int64) - colours).max(axis=0)
        worst = np.maximum(worst, err)
    print("round trip, worst error in (R, G, B):", worst.tolist())
    assert (worst <= (1, 1, 2)).all(), worst


def test_the_three_sitings_on_a_hand_worked_plane():
    """3 x 3 luma pixels over a 2 x 2 chroma plane, by hand from the header's rule"""
    c = np.array([[0, 16], [32, 48]])
    assert ref.upsample(c, 3, 3, "nearest").tolist() == [[0, 0, 16], [0, 0, 16], [32, 32, 48]]
    # centre, pixel (1, 1): j = i = 0, j' = i' = 1: (9 * 0 + 3 * 16 + 3 * 32 + 48 + 8) >> 4 = 12
    # pixel (0, 0): j' = i' = -1, clamped to 0: C[0][0] = 0;  pixel (2, 2): j = i = 1, j' = i' = 0: (9 * 48 + 48 + 96 + 0 + 8) >> 4 = 36
    got = ref.upsample(c, 3, 3, "center")
    assert (got[1, 1], got[0, 0], got[2, 2]) == (12, 0, 36)
    # left, pixel (1, 0): x even: (3 * 0 + 32 + 2) >> 2 = 8;  pixel (1, 1): x odd: (0 + 3 * 16 + 32 + 48 + 4) >> 3 = 16
    got = ref.upsample(c, 3, 3, "left")
    assert (got[1, 0], got[1, 1], got[0, 0]) == (8, 16, 0)


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_the_entry_points_and_abi_is_unchanged():
    from tooncrafter_amd import _lib
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"#define\s+TC_ABI_VERSION\s+14\b", header) and _lib.TC_ABI_VERSION == 14
    assert re.search(r"\bint\s+tc_yuv_matrix\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\[7\]\s*\)\s*;", header)
    assert re.search(r"\bint\s+tc_frames_from_yuv\s*\(\s*const\s+TcFramesYuvParams\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"\bint64_t\s+tc_frames_from_yuv_workspace\s*\(\s*const\s+TcFramesYuvParams\s*\*", header)
    for name, value in (("TC_PIXFMT_I420", 1), ("TC_PIXFMT_NV12", 2), ("TC_PIXFMT_P010", 3), ("TC_CHROMA_NEAREST", 0), ("TC_CHROMA_CENTER", 1),
                        ("TC_CHROMA_LEFT", 2), ("TC_YUV_BT601", 0), ("TC_YUV_BT709", 1), ("TC_YUV_LIMITED", 0), ("TC_YUV_FULL", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert _lib.TC_YUV_FORMATS == ref.FORMATS and _lib.TC_CHROMA_SITINGS == {s: i for i, s in enumerate(ref.SITINGS)}
    assert _lib.TC_YUV_STANDARDS == {"bt601": 0, "bt709": 1} and _lib.TC_YUV_RANGES == {"limited": 0, "full": 1}


def test_ctypes_struct_matches_the_compiled_header(tmp_path):
    """A probe compiled against the header prints sizeof and every offsetof; the ctypes mirror must agree."""
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcFramesYuvParams._fields_) == YUV_FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %zu %zu", TC_ABI_VERSION, sizeof(TcFramesYuvParams), sizeof(((TcFramesYuvParams*)0)->m));']
    lines += [f'  printf(" %zu", offsetof(TcFramesYuvParams, {f}));' for f in YUV_FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:3] == [14, ctypes.sizeof(_lib.TcFramesYuvParams), 28]
    assert got[3:] == [getattr(_lib.TcFramesYuvParams, f).offset for f in YUV_FIELDS]


def test_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build, clip
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ("tc_yuv_matrix", "tc_frames_from_yuv_workspace", "tc_frames_from_yuv"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_frames_from_yuv"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcFramesYuvParams), ctypes.c_void_p])
    assert _lib.load().tc_abi_version() == 14
    assert callable(HipOps.frames_from_yuv) and callable(HipOps.yuv_matrix) and TorchLibOps.frames_from_yuv is not HipOps.frames_from_yuv
    for name in ("Planes", "planes_from_packed", "frames_from_planes", "synthesize_timeline_u8"):
        assert callable(getattr(clip, name)), name
    assert callable(clip.Conditions.from_planes)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_frames_from_yuv_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    n, sh, sw, ch, cw = 2, 37, 53, 19, 27                                         # 37 x 53 -> 16 x 22 for a 16 x 24 target
    py, pc = 120, 112                                                             # pitches that hold a P010 row (106 / 108 bytes) too
    ybuf = (ctypes.c_uint8 * (n * sh * py))()
    cbuf = (ctypes.c_uint8 * (n * ch * pc))()
    c1buf = (ctypes.c_uint8 * (n * ch * pc))()
    out = (ctypes.c_float * (2 * 3 * 4 * 16 * 24))()
    tab = (ctypes.c_int32 * 256)()
    ws = (ctypes.c_uint8 * (1 << 16))()
    slots = (ctypes.c_int32 * 2)(0, 7)
    need = n * sh * sw * 3 + n * sh * 22 * 3
    I420, NV12, P010 = 1, 2, 3

    def params(**kw):
        p = _lib.TcFramesYuvParams(y=ctypes.addressof(ybuf), c0=ctypes.addressof(cbuf), image_stride_y=sh * py, image_stride_c=ch * pc,
                                   pitch_y=py, pitch_c=pc, format=NV12, siting=1, m=(ctypes.c_int32 * 7)(76309, 104597, 25675, 53279, 132201, 16, 128),
                                   n=n, sh=sh, sw=sw, slots=slots, out=ctypes.addressof(out), b=2, t=4, h=16, w=24, h_kmax=7, v_kmax=7,
                                   workspace=ctypes.addressof(ws), workspace_bytes=len(ws))
        p.h_bounds = p.h_coefs = p.v_bounds = p.v_coefs = ctypes.addressof(tab)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rc(**kw):
        return lib.tc_frames_from_yuv(ctypes.byref(params(**kw)), None)
    c1 = ctypes.addressof(c1buf)
    assert lib.tc_frames_from_yuv(None, None) == -1 and lib.tc_frames_from_yuv_workspace(None) == 0
    assert rc(y=None) == -1 and rc(c0=None) == -1 and rc(out=None) == -1 and rc(slots=None) == -1
    assert rc(format=I420) == -1 and rc(format=NV12, c1=c1) == -1 and rc(format=P010, c1=c1) == -1      # c1: I420, and only I420
    assert rc(format=0) == -1 and rc(format=4) == -1 and rc(format=-1) == -1      # RGB24 is not a planar source
    assert rc(siting=3) == -1 and rc(siting=-1) == -1
    assert rc(n=0) == -1 and rc(n=-2) == -1 and rc(n=_lib.TC_FRAMES_U8_MAX + 1) == -1
    assert rc(sh=0) == -1 and rc(sw=0) == -1 and rc(h=0) == -1 and rc(w=-3) == -1 and rc(b=0) == -1 and rc(t=0) == -1
    assert rc(pitch_y=sw - 1) == -1 and rc(format=P010, pitch_y=2 * sw - 2) == -1
    assert rc(format=I420, c1=c1, pitch_c=cw - 1) == -1 and rc(pitch_c=2 * cw - 1) == -1 and rc(format=P010, pitch_c=4 * cw - 2) == -1
    assert rc(image_stride_y=sh * py - 1) == -1 and rc(image_stride_c=ch * pc - 1) == -1
    assert rc(slots=(ctypes.c_int32 * 2)(0, 8)) == -1 and rc(slots=(ctypes.c_int32 * 2)(-1, 3)) == -1
    assert rc(h_coefs=None) == -1 and rc(v_bounds=None) == -1 and rc(v_kmax=0) == -1      # resized, but a table is missing
    zero_cy, neg_cy = (ctypes.c_int32 * 7)(0, 1, 1, 1, 1, 16, 128), (ctypes.c_int32 * 7)(-5, 1, 1, 1, 1, 16, 128)
    assert rc(m=zero_cy) == -1 and rc(m=neg_cy) == -1
    # P010: words, so pointers, pitches and image strides are even
    assert rc(format=P010, y=ctypes.addressof(ybuf) + 1) == -2 and rc(format=P010, c0=ctypes.addressof(cbuf) + 1) == -2
    assert rc(format=P010, pitch_y=py - 1, image_stride_y=sh * py) == -2 and rc(format=P010, pitch_c=pc - 1) == -2
    assert rc(format=P010, image_stride_y=sh * py + 1) == -2
    # the 8-bit formats have no alignment rule: an odd pointer and pitch get as far as the workspace check
    assert rc(y=ctypes.addressof(ybuf) + 1, pitch_y=py - 1, pitch_c=pc - 1, workspace_bytes=need - 1) == -4
    # the RGB image, plus tc_frames_from_u8's intermediate for the same sizes
    assert lib.tc_frames_from_yuv_workspace(ctypes.byref(params())) == need
    p = params(sh=16, sw=40)                                                      # nothing to resize: the RGB image alone
    assert lib.tc_frames_from_yuv_workspace(ctypes.byref(p)) == n * 16 * 40 * 3
    assert rc(workspace=None) == -4 and rc(workspace_bytes=need - 1) == -4
    assert rc(format=I420, c1=c1, workspace_bytes=need - 1) == -4 and rc(format=P010, workspace_bytes=need - 1) == -4
    assert not any(out) and not any(tab) and not any(ws)


# ---------------------------------------------------------------- the operator layer and the Python interface

def test_meta_kernel_infers_the_clip_shape():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    assert str(t.frames_from_yuv.default._schema).startswith(
        "tooncrafter::frames_from_yuv(Tensor y, Tensor c0, Tensor? c1, int format, int[] m, int siting, int[] slots, int b, int t, int h, int w,")
    m = ref.matrix("bt601", "limited", 8)
    def tabs(n_out):                                      # the tables of one resized axis: a row per output index
        return torch.empty(n_out, 2, dtype=torch.int32, device="meta"), torch.empty(n_out, 4, dtype=torch.int32, device="meta")
    from tooncrafter_amd import _lib
    rh, rw = ctypes.c_int32(), ctypes.c_int32()               # (37, 53) images are resized to (rh, rw) on the way to (16, 24)
    assert _lib.load().tc_frames_from_u8_resized(37, 53, 16, 24, ctypes.byref(rh), ctypes.byref(rw)) == 0
    assert (rh.value, rw.value) != (37, 53)
    y = torch.empty(2, 37, 53, dtype=torch.uint8, device="meta")
    c = torch.empty(2, 19, 27, dtype=torch.uint8, device="meta")
    cc = torch.empty(2, 19, 27, 2, dtype=torch.uint8, device="meta")
    for args in ((y, c, c, 1), (y, cc, None, 2), (y.to(torch.int16), cc.to(torch.int16), None, 3)):
        out = t.frames_from_yuv(*args, m, 1, [0, 3], 1, 4, 16, 24, *tabs(rw.value), *tabs(rh.value))
        assert out.shape == (1, 3, 4, 16, 24) and out.dtype == torch.float32 and out.device.type == "meta"
        for tables in ((None,) * 4, tabs(4) * 2):             # a resize without its tables: refused as on the CUDA key
            with pytest.raises(RuntimeError, match="tables of"):
                t.frames_from_yuv(*args, m, 1, [0, 3], 1, 4, 16, 24, *tables)
    y, cc = torch.empty(2, 16, 24, dtype=torch.uint8, device="meta"), torch.empty(2, 8, 12, 2, dtype=torch.uint8, device="meta")
    for tables in ((None,) * 4, tabs(4) * 2):                 # images of the frame size keep it: the tables are not looked at
        out = t.frames_from_yuv(y, cc, None, 2, m, 1, [0, 3], 1, 4, 16, 24, *tables)
        assert out.shape == (1, 3, 4, 16, 24) and out.dtype == torch.float32 and out.device.type == "meta"
    with pytest.raises((RuntimeError, NotImplementedError)):                      # no CPU kernel is registered: no fallback
        t.frames_from_yuv(torch.zeros(1, 4, 6, dtype=torch.uint8), torch.zeros(1, 2, 3, 2, dtype=torch.uint8), None, 2, m, 1, [0], 1, 1,
                          16, 24, None, None, None, None)


def test_planes_reject_wrong_dtypes_shapes_and_strides():
    from tooncrafter_amd import clip
    from tooncrafter_amd._lib import TooncrafterHipError
    u8 = torch.uint8
    y, cb, cc = torch.zeros(2, 5, 7, dtype=u8), torch.zeros(2, 3, 4, dtype=u8), torch.zeros(2, 3, 4, 2, dtype=u8)
    ok = [clip.Planes(y, (cb, cb.clone()), "i420"), clip.Planes(y, (cc,), "nv12"), clip.Planes(y, cc, "nv12"),
          clip.Planes(y.to(torch.int16), (cc.to(torch.int16),), "p010"), clip.Planes(y.to(torch.uint16), (cc.to(torch.uint16),), "p010"),
          clip.Planes(torch.zeros(2, 5, 16, dtype=u8)[:, :, :7], (torch.zeros(2, 3, 16, 2, dtype=u8)[:, :, :4],), "nv12")]     # pitched rows
    assert [len(p) for p in ok] == [2] * 6 and len(ok[0][1:]) == 1 and ok[1][0:1].y.data_ptr() == y.data_ptr()
    bad = [
        (y.float(), (cc,), "nv12"), (y, (cc.to(torch.int16),), "nv12"), (y, (cc,), "p010"), (y.to(torch.int32), (cc.to(torch.int32),), "p010"),
        (y, (cb,), "i420"), (y, (cb, cb, cb), "i420"), (y, (cc, cc), "nv12"), (y, (cb, cb), "nv12"),      # plane counts and shapes per format
        (y[0], (cc,), "nv12"), (y, (cc[:, :2],), "nv12"), (y, (cc[:, :, :3],), "nv12"), (y, (cc[:1],), "nv12"), (y, (cb, cb[:, :, :3]), "i420"),
        (torch.zeros(2, 7, 8, dtype=u8), (cc,), "nv12"), (torch.zeros(2, 6, 9, dtype=u8), (cc,), "nv12"),      # chroma of a 5 x 7 picture
        (torch.zeros(2, 5, 14, dtype=u8)[:, :, ::2], (cc,), "nv12"),                                       # stride two inside a row
        (y, (torch.zeros(2, 3, 4, 4, dtype=u8)[..., ::2],), "nv12"), (y, (torch.zeros(2, 3, 8, 2, dtype=u8)[:, :, ::2],), "nv12"),
        (y.permute(0, 2, 1).contiguous().permute(0, 2, 1), (cc,), "nv12"),                                 # column-major
        (y, (cb, torch.zeros(2, 3, 8, dtype=u8)[:, :, :4]), "i420"),                                       # Cb and Cr pitched differently
        (y.expand(2, 5, 7)[:1].expand(2, 5, 7), (cc,), "nv12"),                                            # images that overlap
        (y, (cc,), "yuy2"), (y, (cc,), "rgb24"), ("frame", (cc,), "nv12"),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            clip.Planes(*args)
    for kw in (dict(standard="bt2020"), dict(range="studio"), dict(siting="top")):
        with pytest.raises(ValueError):
            clip.Planes(y, (cc,), "nv12", **kw)
    good = ok[1]
    for slots in ([(0, 0)], [(0, 0), (0, 4)], [(0, 0), (-1, 1)], [(0, 0), (0, 1), (0, 2)]):
        with pytest.raises(ValueError):
            clip.frames_from_planes(good, (16, 24), slots, 4)
    with pytest.raises(ValueError):
        clip.frames_from_planes(good, (16, 0), [(0, 0), (0, 3)], 4)
    with pytest.raises(ValueError):
        clip.frames_from_planes(y, (16, 24), [(0, 0), (0, 3)], 4)                 # a tensor is not a Planes
    with pytest.raises(ValueError):
        clip.Conditions.from_planes(None, good, good[:1], size=(16, 24), t=4)     # one last frame for two first frames
    with pytest.raises(ValueError):
        clip.Conditions.from_planes(None, good, y, size=(16, 24), t=4)
    with pytest.raises(ValueError):                                               # a matrix of six entries
        clip.Planes(y, (cc,), "nv12", matrix=[1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError):                                               # cy = 0
        clip.Planes(y, (cc,), "nv12", matrix=[0, 2, 3, 4, 5, 16, 128])
    with pytest.raises(TooncrafterHipError):                                      # well-formed CPU planes: no fallback
        clip.frames_from_planes(good, (16, 24), [(0, 0), (0, 3)], 4)


def test_planes_from_packed_returns_views_of_the_buffer():
    from tooncrafter_amd import clip
    h, w = 6, 8
    frame = h * w * 3 // 2
    buf = torch.arange(2 * 3 * frame, dtype=torch.int32).to(torch.uint8).view(2, 3, frame)      # (b, t, bytes), as clip_to_uint8 returns
    np_buf = buf.numpy()
    for fmt in ("i420", "nv12"):
        p = clip.planes_from_packed(buf, h, w, fmt)
        assert len(p) == 6 and p.fmt == fmt and (p.standard, p.range, p.siting) == ("bt601", "limited", "center")
        assert p.y.shape == (6, h, w) and p.y.data_ptr() == buf.data_ptr()
        flat = np_buf.reshape(6, frame)
        assert np.array_equal(p.y.numpy(), flat[:, :h * w].reshape(6, h, w))
        if fmt == "i420":
            assert [tuple(c.shape) for c in p.chroma] == [(6, 3, 4)] * 2
            assert np.array_equal(p.chroma[0].numpy(), flat[:, 48:60].reshape(6, 3, 4)) and np.array_equal(p.chroma[1].numpy(), flat[:, 60:].reshape(6, 3, 4))
            assert p.chroma[1].data_ptr() == buf.data_ptr() + 60
        else:
            assert [tuple(c.shape) for c in p.chroma] == [(6, 3, 4, 2)]
            assert np.array_equal(p.chroma[0].numpy(), flat[:, 48:].reshape(6, 3, 4, 2)) and p.chroma[0].data_ptr() == buf.data_ptr() + 48
        buf[1, 2, 0] += 1                                                         # shared storage: a write shows through
        assert p.y[5, 0, 0] == buf[1, 2, 0]
        last = clip.planes_from_packed(buf[:, -1], h, w, fmt, siting="nearest")   # the last frame of every clip, still a view
        assert len(last) == 2 and last.y.data_ptr() == buf[0, 2].data_ptr() and last.siting == "nearest"
    # what it writes is what the back end's statement lays out
    rgb = np.random.default_rng(3).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    for fmt in ("i420", "nv12"):
        p = clip.planes_from_packed(torch.from_numpy(back.packed(rgb, fmt)), h, w, fmt)
        y, cb, cr = back.yuv420(rgb)
        got = ref.samples((p.y.numpy(),) + tuple(c.numpy() for c in p.chroma), fmt)
        assert all(np.array_equal(a, b) for a, b in zip(got, (y, cb, cr)))
    for bad in ((buf, 5, 8, "i420"), (buf, 6, 7, "nv12"), (buf, 6, 8, "p010"), (buf, 6, 10, "i420"), (buf.float(), 6, 8, "i420"),
                (buf[:, :, ::2], 6, 8, "i420"), (buf.transpose(0, 1), 6, 8, "nv12"), ("frames", 6, 8, "nv12")):
        with pytest.raises(ValueError):
            clip.planes_from_packed(*bad)


# ---------------------------------------------------------------- the timeline's splice arithmetic, on a stub model

class StubOps:
    """frames_to_u8 by the back end's numpy statement, into the caller's buffer at the caller's strides"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def clip_seeds(seeds, b, what="seeds"):
        from tooncrafter_amd import ops
        return ops.clip_seeds(seeds, b, what)

    def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
        f0, nf = frames
        pitch, frame_stride, clip_stride = strides
        self.calls.append((x.shape[0], f0, nf))
        u8 = back.to_u8(x.numpy())[:, f0:f0 + nf]                                 # (b, nf, h, w, 3)
        if size is not None:
            u8 = back.resize(u8, size[0], size[1], filter)
        dst = out.numpy()
        assert (x.shape[0] - 1) * clip_stride + (nf - 1) * frame_stride + back.frame_bytes(fmt, u8.shape[2], pitch) <= dst.size
        for i in range(u8.shape[0]):
            for j in range(nf):
                back.place(dst[i * clip_stride + j * frame_stride:], u8[i, j], fmt, pitch)
        return out


@pytest.mark.parametrize("fmt", ["rgb24", "i420", "nv12"])
@pytest.mark.parametrize("k,t", [(2, 4), (3, 4), (5, 4), (2, 16), (3, 16), (5, 16)])
def test_timeline_splice_counts_and_offsets(monkeypatch, k, t, fmt):
    """Frame (segment s, index f) of the stub's clips is the constant grey 16 * s + f: the video must hold, in order, frames
    0 .. t-1 of segment 0 and frames 1 .. t-1 of every later segment, whatever the batch size."""
    from tooncrafter_amd import clip, output
    h, w = 4, 6
    frame = h * w * 3 if fmt == "rgb24" else h * w * 3 // 2
    total = (k - 1) * (t - 1) + 1
    kf = torch.arange(k, dtype=torch.uint8).view(k, 1, 1, 1).expand(k, 8, 8, 3).contiguous()
    seen = []

    def from_uint8(model, first, last, *, size, t, **options):
        assert torch.equal(last[:, 0, 0, 0], first[:, 0, 0, 0] + 1)                # segment i: keyframe i -> i + 1
        assert options["hold_endpoints"] is True and options["prompts"] is None
        return [int(v) for v in first[:, 0, 0, 0]]                               # the batch's segments stand in for the conditions

    def sample(model, cond, plan, latent_shape, pinned=None, variant=0):
        assert latent_shape[0] == len(cond) and list(plan.seeds) == [100 + s for s in cond]
        seen.append(list(cond))
        return cond

    def decode_spliced(model, segs, refs):
        grey = torch.tensor([[16 * s + f for f in range(t)] for s in segs], dtype=torch.float32)     # (n, t)
        return ((grey + 0.5) / 255 * 2 - 1).view(len(segs), 1, t, 1, 1).expand(len(segs), 3, t, h, w).contiguous()

    class Cond(list):
        refs = None
    monkeypatch.setattr(clip.Conditions, "from_uint8", staticmethod(lambda *a, **kw: Cond(from_uint8(*a, **kw))))
    monkeypatch.setattr(clip, "sample", sample)
    monkeypatch.setattr(clip, "decode_spliced", decode_spliced)
    want_grey = list(range(t)) + [16 * s + f for s in range(1, k - 1) for f in range(1, t)]
    assert len(want_grey) == total
    for batch in (1, 2, 3):
        stub = StubOps()
        monkeypatch.setattr(clip, "ops", stub)
        monkeypatch.setattr(output, "ops", stub)                                # the writer rule lives there
        seen.clear()
        plan = clip.SamplingPlan(steps=2, seeds=[100 + s for s in range(k - 1)])
        video = clip.synthesize_timeline_u8(None, kf, [batch, 4, t, 1, 1], size=(h, w), plan=plan, out_fmt=fmt)
        assert video.shape == ((total, h, w, 3) if fmt == "rgb24" else (total, frame)) and video.dtype == torch.uint8
        assert seen == [list(range(i, min(i + batch, k - 1))) for i in range(0, k - 1, batch)]
        assert clip.timeline_layout(k, t, batch, (h, w), fmt) == (total, frame, [(s[0], len(s)) for s in seen])
        want = np.stack([back.packed(np.full((h, w, 3), g, np.uint8), fmt) for g in want_grey])
        assert np.array_equal(video.numpy().reshape(total, -1), want.reshape(total, -1)), (batch, stub.calls)
        # every byte was written exactly once: the first frame alone, then t - 1 frames per segment
        assert sum(b * nf for b, _, nf in stub.calls) == total and stub.calls[0] == (1, 0, 1)


def test_timeline_rejects_bad_requests():
    from tooncrafter_amd import clip
    kf = torch.zeros(3, 8, 8, 3, dtype=torch.uint8)
    plan = clip.SamplingPlan(steps=2)
    for bad in (dict(keyframes=kf[:1]), dict(keyframes=kf.float()), dict(keyframes=kf[..., :2]), dict(out_fmt="p010"),
                dict(out_fmt="i420", out_size=(5, 6)), dict(prompts=["a"]), dict(plan=clip.SamplingPlan(steps=2, seeds=[1])),
                dict(plan=clip.SamplingPlan(steps=2, seeds=[1, 2, 3]))):
        kw = dict(keyframes=kf, size=(4, 6), plan=plan)
        kw.update(bad)
        with pytest.raises(ValueError):
            clip.synthesize_timeline_u8(None, kw.pop("keyframes"), [1, 4, 4, 1, 1], **kw)
    assert clip.timeline_layout(4, 4, 2, (4, 6), "rgb24") == (10, 72, [(0, 2), (2, 1)])
