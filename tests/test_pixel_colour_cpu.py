"""Planar frames out in a named colour, without a GPU (tc_yuv_out_matrix, tc_frames_to_yuv; additive within ABI 14): the host
matrix builder equals the numpy statement of tests/pixel_colour_ref.py and the issue's check points, and the statement stays
within one code value of the standards' float64 formulas; the struct has the header's layout, the symbols are exported and
bound, the Meta kernel infers shapes; every documented refusal returns before any device call; the 16-bit resample statement
equals PIL's float resize within its rounding; `Colour`, the `colour=` keywords, `timeline_layout` and `planes_from_frames`
behave as documented and `colour=None` is the old call; the .mp4 says what its planes are.  Compute is covered by
tests/test_gpu_pixel_colour.py."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import pixel_back_ref as back
import pixel_colour_ref as ref
from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
YUV_OUT_FIELDS = ("x", "out", "b", "t", "h", "w", "f0", "nf", "oh", "ow", "format", "pitch", "frame_stride", "clip_stride",
                  "h_bounds", "h_coefs", "h_kmax", "v_bounds", "v_coefs", "v_kmax", "workspace", "workspace_bytes", "siting", "m")
ENTRY_POINTS = ("tc_yuv_out_matrix", "tc_frames_to_yuv_workspace", "tc_frames_to_yuv")
CASES = [(s, r, b) for s in ("bt601", "bt709") for r in ("limited", "full") for b in (8, 10)]
STD, RNG = {"bt601": 0, "bt709": 1}, {"limited": 0, "full": 1}


def c_matrix(lib, standard, range_, bits):
    m = (ctypes.c_int32 * 11)(*([-7] * 11))
    assert lib.tc_yuv_out_matrix(STD[standard], RNG[range_], bits, m) == 0
    return list(m)


# ---------------------------------------------------------------- the matrix

def test_out_matrix_equals_the_statement_and_the_check_points():
    from tooncrafter_amd import _lib
    from tooncrafter_amd.ops import HipOps
    lib = _lib.load()
    for case in CASES:
        m = c_matrix(lib, *case)
        assert m == ref.out_matrix(*case), case
        assert sum(m[3:6]) == 0 and sum(m[6:9]) == 0, case                        # grey is exactly neutral
        assert m[5] == m[6] and min(m[:3]) > 0
        assert HipOps().yuv_out_matrix(*case) == m
    for case, want in ref.TABLE.items():
        assert c_matrix(lib, *case) == want, case
    # the BT.601 limited 8-bit row is the nine constants tc_frames_to_u8's header block states
    with open(HEADER) as f:
        header = f.read()
    doc = header[header.index("Pixel back end"):header.index("int tc_frames_to_u8(")]
    for v in ref.TABLE[("bt601", "limited", 8)][:9]:
        assert str(abs(v)) in doc, v
    # refusals
    m = (ctypes.c_int32 * 11)()
    assert lib.tc_yuv_out_matrix(0, 0, 8, None) == -1
    for bad in ((2, 0, 8), (-1, 0, 8), (0, 2, 8), (0, -1, 10), (0, 0, 9), (1, 1, 16), (0, 0, 0)):
        assert lib.tc_yuv_out_matrix(*bad, m) == -1, bad
    assert not any(m)
    for bad in (("bt2020", "limited", 8), ("bt709", "video", 8)):
        with pytest.raises(ValueError):
            HipOps().yuv_out_matrix(*bad)
    with pytest.raises(_lib.TooncrafterHipError):
        HipOps().yuv_out_matrix("bt709", "limited", 12)


def test_reference_colours():
    """the issue's points: BT.709 limited red, white and black at both depths"""
    def codes(rgb, case):
        bits = case[2]
        px = np.array(rgb, np.uint16 if bits == 10 else np.uint8).reshape(1, 1, 3).repeat(2, 0).repeat(2, 1)
        y, cb, cr = ref.yuv420(px, ref.out_matrix(*case), "center", bits)
        left = ref.yuv420(px, ref.out_matrix(*case), "left", bits)
        assert all(np.array_equal(a, b) for a, b in zip((y, cb, cr), left))       # a flat block: the siting does not matter
        return int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])
    assert codes((255, 0, 0), ("bt709", "limited", 8)) == (63, 102, 240)
    assert codes((65535, 0, 0), ("bt709", "limited", 10)) == (250, 409, 960)
    assert codes((65535,) * 3, ("bt709", "limited", 10)) == (940, 512, 512)
    assert codes((0, 0, 0), ("bt709", "limited", 10)) == (64, 512, 512)
    assert codes((255,) * 3, ("bt601", "limited", 8)) == (235, 128, 128) and codes((0, 0, 0), ("bt601", "limited", 8)) == (16, 128, 128)
    assert codes((255, 0, 0), ("bt601", "limited", 8))[0] == 81 and codes((0, 0, 255), ("bt601", "limited", 8))[0] == 41
    assert codes((0, 0, 255), ("bt601", "full", 8))[1] == 255                     # 256 before the clip
    assert codes((0, 0, 65535), ("bt709", "full", 10))[1] == 1023


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_the_fixed_point_stays_within_one_code_value_of_the_standard(case):
    """a colour grid and the eight cube corners as flat 2 x 2 blocks, both sitings: |integer - float64| <= 1 after the float
    value is clipped to the code range (the issue measured 0.51 at most)"""
    bits = case[2]
    top_in = 255 if bits == 8 else 65535
    v = np.unique(np.concatenate([np.linspace(0, top_in, 18).round(), [1, top_in - 1]])).astype(np.int64)
    grid = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 1, 3)      # (n, 1, 3): corners included
    px = grid.repeat(2, axis=1)[:, None].repeat(2, axis=1).astype(np.uint16 if bits == 10 else np.uint8)      # (n, 2, 2, 3)
    want = [np.clip(c, 0, (1 << bits) - 1) for c in ref.codes_double(grid[:, 0], *case)]
    worst = 0.0
    for siting in ("center", "left"):
        y, cb, cr = ref.yuv420(px, ref.out_matrix(*case), siting, bits)
        for got, w in ((y[:, 0, 0], want[0]), (cb[:, 0, 0], want[1]), (cr[:, 0, 0], want[2])):
            worst = max(worst, float(np.abs(got - w).max()))
    print(f"{case}: worst |integer - float64| = {worst:.4f} code values")
    assert worst <= 1.0


# ---------------------------------------------------------------- declaration, layout, export

def test_ctypes_struct_matches_the_compiled_header(tmp_path):
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcFramesYuvOutParams._fields_) == YUV_OUT_FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %zu %zu", TC_ABI_VERSION, sizeof(TcFramesYuvOutParams), sizeof(((TcFramesYuvOutParams*)0)->m));']
    lines += [f'  printf(" %zu", offsetof(TcFramesYuvOutParams, {f}));' for f in YUV_OUT_FIELDS]
    lines += ['  printf(" %d %d %d %d %d", TC_PIXFMT_I420, TC_PIXFMT_NV12, TC_PIXFMT_P010, TC_CHROMA_CENTER, TC_CHROMA_LEFT);', '  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:3] == [14, ctypes.sizeof(_lib.TcFramesYuvOutParams), 44]
    assert got[3:-5] == [getattr(_lib.TcFramesYuvOutParams, f).offset for f in YUV_OUT_FIELDS]
    assert got[-5:] == [ref.FORMATS["i420"], ref.FORMATS["nv12"], ref.FORMATS["p010"], ref.SITINGS["center"], ref.SITINGS["left"]]
    assert (_lib.TC_YUV_FORMATS, _lib.TC_CHROMA_SITINGS["center"], _lib.TC_CHROMA_SITINGS["left"]) == (ref.FORMATS, 1, 2)
    assert _lib.TC_PIXFMTS == {"rgb24": 0, "i420": 1, "nv12": 2}                  # fmt="p010" stays refused: 10 bits is a colour's


def test_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_frames_to_yuv"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcFramesYuvOutParams), ctypes.c_void_p])
    assert _lib.SYMBOLS["tc_frames_to_yuv_workspace"] == (ctypes.c_int64, [ctypes.POINTER(_lib.TcFramesYuvOutParams)])
    assert _lib.load().tc_abi_version() == 14 and _lib.TC_ABI_VERSION == 14
    assert callable(HipOps.frames_to_yuv) and TorchLibOps.frames_to_yuv is not HipOps.frames_to_yuv
    with open(HEADER) as f:
        header = f.read()
    assert "int tc_frames_to_yuv(const TcFramesYuvOutParams* p, void* stream);" in header
    assert "int tc_yuv_out_matrix(int32_t standard, int32_t range, int32_t bits, int32_t m[11]);" in header


def test_meta_kernel_infers_shape_and_dtype():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    assert str(t.frames_to_yuv.default._schema).startswith(
        "tooncrafter::frames_to_yuv(Tensor x, int oh, int ow, int format, int f0, int nf, int siting, int[] m,")
    x = torch.empty(2, 3, 5, 20, 32, device="meta")
    def tabs(n_out):                                      # the tables of one resized axis: a row per output index
        return torch.empty(n_out, 2, dtype=torch.int32, device="meta"), torch.empty(n_out, 4, dtype=torch.int32, device="meta")
    m = ref.out_matrix("bt709", "limited", 8)
    for fmt, scale in ((1, 1), (2, 1), (3, 2)):
        y = t.frames_to_yuv(x, 46, 72, fmt, 1, 3, 2, m, *tabs(72), *tabs(46))      # (20, 32) -> (46, 72): w -> ow, then h -> oh
        assert y.shape == (2, 3, 46 * 72 * 3 // 2 * scale) and y.dtype == torch.uint8 and y.device.type == "meta"
        y = t.frames_to_yuv(x, 20, 72, fmt, 1, 3, 2, m, *tabs(72), None, None)      # None for the axis that keeps its size
        assert y.shape == (2, 3, 20 * 72 * 3 // 2 * scale) and y.dtype == torch.uint8 and y.device.type == "meta"
        for tables in ((None,) * 4, tabs(4) * 2):                                  # a resize without its tables: refused as on the CUDA key
            with pytest.raises(RuntimeError, match="tables of"):
                t.frames_to_yuv(x, 46, 72, fmt, 1, 3, 2, m, *tables)
    for bad in ((45, 72, 1, 0, 5, 1, m), (46, 71, 2, 0, 5, 1, m), (46, 72, 0, 0, 5, 1, m), (46, 72, 4, 0, 5, 1, m), (46, 72, 2, 3, 3, 1, m),
                (46, 72, 2, 0, 5, 0, m), (46, 72, 2, 0, 5, 3, m), (46, 72, 2, 0, 5, 1, m[:7])):
        with pytest.raises(RuntimeError):
            t.frames_to_yuv(x, *bad, None, None, None, None)
    with pytest.raises((RuntimeError, NotImplementedError)):                      # no CPU kernel is registered: no fallback
        t.frames_to_yuv(torch.zeros(1, 3, 2, 20, 32), 20, 32, 2, 0, 2, 1, m, None, None, None, None)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_frames_to_yuv_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    x = (ctypes.c_float * (2 * 3 * 3 * 20 * 32))()
    out = (ctypes.c_uint16 * (2 * 3 * 46 * 72 * 3 // 2))()                        # 2-byte aligned
    tab = (ctypes.c_int32 * 1024)()
    ws = (ctypes.c_uint16 * 64)()
    m = ref.out_matrix("bt709", "limited", 8)
    fb = 46 * 72 * 3 // 2

    def params(**kw):
        p = _lib.TcFramesYuvOutParams(x=ctypes.addressof(x), out=ctypes.addressof(out), b=2, t=3, h=20, w=32, f0=0, nf=3, oh=46, ow=72,
                                      format=2, pitch=72, frame_stride=fb, clip_stride=3 * fb, h_kmax=5, v_kmax=5, siting=2,
                                      m=(ctypes.c_int32 * 11)(*m))
        p.h_bounds = p.h_coefs = p.v_bounds = p.v_coefs = ctypes.addressof(tab)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rc(**kw):
        return lib.tc_frames_to_yuv(ctypes.byref(params(**kw)), None)
    p010 = dict(format=3, pitch=144, frame_stride=2 * fb, clip_stride=6 * fb, m=(ctypes.c_int32 * 11)(*ref.out_matrix("bt709", "limited", 10)))
    n = 2 * 3
    need = n * 20 * 32 * 3 + n * 20 * 72 * 3
    assert lib.tc_frames_to_yuv(None, None) == -1 and lib.tc_frames_to_yuv_workspace(None) == 0
    assert rc() == -4 and rc(**p010) == -4 and rc(format=1) == -4 and rc(siting=1) == -4       # well formed: on to the workspace
    assert rc(x=None) == -1 and rc(out=None) == -1
    for name in ("b", "t", "h", "w", "oh", "ow"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -2}) == -1, name
    assert rc(f0=-1) == -1 and rc(nf=0) == -1 and rc(f0=1) == -1 and rc(nf=4) == -1
    assert rc(format=0) == -1 and rc(format=4) == -1 and rc(format=-1) == -1      # RGB24 is tc_frames_to_u8's
    assert rc(siting=0) == -1 and rc(siting=3) == -1                              # NEAREST does not produce chroma
    for i in range(3):
        for v in (0, -5):
            bad = list(m)
            bad[i] = v
            assert rc(m=(ctypes.c_int32 * 11)(*bad)) == -1, (i, v)
    assert rc(oh=45) == -3 and rc(ow=71) == -3 and rc(**dict(p010, oh=45)) == -3 and rc(format=1, ow=71) == -3      # odd sizes
    assert rc(format=1, pitch=73) == -3                                           # I420: Cb rows pitch / 2 apart
    assert rc(pitch=71) == -1 and rc(**dict(p010, pitch=142)) == -1               # a row does not hold its samples
    assert rc(frame_stride=fb - 1) == -1 and rc(**dict(p010, frame_stride=2 * fb - 2)) == -1
    assert rc(clip_stride=3 * fb - 1) == -1 and rc(b=1, clip_stride=0) == -4
    assert rc(h_coefs=None) == -1 and rc(h_bounds=None) == -1 and rc(v_bounds=None) == -1 and rc(v_coefs=None) == -1
    assert rc(h_kmax=0) == -1 and rc(v_kmax=-1) == -1
    # P010: everything in whole 2-byte words
    wide_pitch = dict(p010, pitch=145, frame_stride=145 * 69, clip_stride=3 * 145 * 69 + 1)
    assert rc(**wide_pitch) == -2
    assert rc(**dict(p010, frame_stride=2 * fb + 1, clip_stride=3 * (2 * fb + 1) + 1)) == -2
    assert rc(**dict(p010, clip_stride=6 * fb + 1)) == -2
    assert rc(**dict(p010, out=ctypes.addressof(out) + 1)) == -2
    assert rc(**dict(p010, workspace=ctypes.addressof(ws) + 1, workspace_bytes=1 << 30)) == -2
    assert rc(pitch=73, frame_stride=73 * 69, clip_stride=3 * 73 * 69) == -4      # 8-bit NV12 takes an odd pitch
    # workspace: 8 bit as tc_frames_to_u8's planar case, P010 two bytes per sample; 0 for a refused request
    assert lib.tc_frames_to_yuv_workspace(ctypes.byref(params())) == need
    assert lib.tc_frames_to_yuv_workspace(ctypes.byref(params(**p010))) == 2 * need
    assert lib.tc_frames_to_yuv_workspace(ctypes.byref(params(f0=1, nf=2, clip_stride=2 * fb))) == 4 * (20 * 32 * 3 + 20 * 72 * 3)
    ident = dict(oh=20, ow=32, pitch=32, frame_stride=960, clip_stride=3 * 960)
    assert lib.tc_frames_to_yuv_workspace(ctypes.byref(params(**ident))) == n * 20 * 32 * 3
    assert lib.tc_frames_to_yuv_workspace(ctypes.byref(params(**dict(p010, oh=20, ow=32, pitch=64, frame_stride=1920, clip_stride=3 * 1920)))) == n * 20 * 32 * 6
    vonly = dict(p010, ow=32, pitch=64, frame_stride=46 * 96, clip_stride=3 * 46 * 96)
    assert lib.tc_frames_to_yuv_workspace(ctypes.byref(params(**vonly))) == n * 20 * 32 * 6
    for refused in (dict(format=0), dict(siting=0), dict(oh=45), wide_pitch):
        assert lib.tc_frames_to_yuv_workspace(ctypes.byref(params(**refused))) == 0
    assert rc(workspace=None, workspace_bytes=1 << 30) == -4
    assert rc(workspace=ctypes.addressof(ws), workspace_bytes=need - 1) == -4
    assert rc(**dict(p010, workspace=ctypes.addressof(ws), workspace_bytes=2 * need - 1)) == -4
    assert not any(out) and not any(tab) and not any(ws)


# ---------------------------------------------------------------- the 16-bit resample statement against PIL

@pytest.mark.parametrize("size", [(46, 72), (14, 22)], ids=["46x72", "14x22"])
@pytest.mark.parametrize("name", back.FILTERS)
def test_resample16_statement_equals_pils_float_resize(name, size):
    """PIL resizes mode "F" images in floating point with unquantised coefficients; the statement's integers differ from it by
    their own rounding (0.5), the coefficients' (each within 2^-23 of its real value, kmax of them on samples up to 65535, in
    the second pass on the rounded output of the first) and fp32 slack"""
    Image = pytest.importorskip("PIL.Image")
    u16 = ref.to_u16(load_golden("pixel_back.npz")["x"])                         # (2, 3, 20, 32, 3)
    oh, ow = size
    got = ref.resize16(u16, oh, ow, name)
    kmax = max(back.tables(name, 32, ow)[1].shape[1], back.tables(name, 20, oh)[1].shape[1])
    bound = 0.5 + 65535 * kmax * 2.0 ** -23 + 0.01
    assert bound < 1
    worst = 0.0
    for i in range(2):
        for j in range(3):
            for c in range(3):
                plane = Image.fromarray(u16[i, j, :, :, c].astype(np.float32), mode="F")
                # pass by pass, as the statement rounds: PIL's own two-pass result is not rounded in between
                mid = np.asarray(plane.resize((ow, 20), getattr(Image, name.upper())), np.float64)
                step1 = ref.resample_pass16(u16[i, j, :, :, c], ow, 1, name)
                worst = max(worst, float(np.abs(step1 - np.clip(mid, 0, 65535)).max()))
                full = np.asarray(Image.fromarray(step1.astype(np.float32), mode="F").resize((ow, oh), getattr(Image, name.upper())), np.float64)
                worst = max(worst, float(np.abs(got[i, j, :, :, c].astype(np.float64) - np.clip(full, 0, 65535)).max()))
    print(f"{name} {size}: worst |statement - PIL| = {worst:.4f} of a 16-bit step, bound {bound:.4f}")
    assert worst <= bound


# ---------------------------------------------------------------- the Python surface

def test_colour_validates_and_reads_planes():
    from tooncrafter_amd import clip
    from tooncrafter_amd.output import Colour
    c = Colour()
    assert (c.standard, c.range, c.siting, c.bits) == ("bt601", "limited", "center", 8)
    assert Colour("bt709", "full", "left", 10) == Colour(standard="bt709", range="full", siting="left", bits=10)
    with pytest.raises(Exception):
        c.bits = 10                                                               # frozen
    for bad in (dict(standard="bt2020"), dict(range="pc"), dict(siting="nearest"), dict(siting="top"), dict(bits=12), dict(bits="10"),
                dict(bits=True), dict(standard=None)):
        with pytest.raises(ValueError):
            Colour(**bad)
    y, cbcr = torch.zeros(1, 4, 6, dtype=torch.uint8), torch.zeros(1, 2, 3, 2, dtype=torch.uint8)
    assert Colour.of(clip.Planes(y, (cbcr,), "nv12", "bt709", "limited", "left")) == Colour("bt709", "limited", "left", 8)
    assert Colour.of(clip.Planes(y, (cbcr[..., 0].contiguous(), cbcr[..., 1].contiguous()), "i420")) == Colour()
    wide = clip.Planes(y.to(torch.uint16), (cbcr.to(torch.uint16),), "p010", "bt709", "full", "center")
    assert Colour.of(wide) == Colour("bt709", "full", "center", 10)
    with pytest.raises(ValueError):
        Colour.of(clip.Planes(y, (cbcr,), "nv12", siting="nearest"))
    with pytest.raises(ValueError):
        Colour.of(clip.Planes(y, (cbcr,), "nv12", matrix=[76309, 104597, 25675, 53279, 132201, 16, 128]))
    with pytest.raises(ValueError):
        Colour.of(y)


class Spy:
    """a recording backend with the signatures of the commit before the colour keywords"""
    def __init__(self):
        self.calls = []

    def video_to_uint8(self, video):
        self.calls.append(("video_to_uint8", tuple(video.shape)))
        return torch.zeros(1)

    def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
        self.calls.append(("frames_to_u8", tuple(x.shape), size, filter, fmt, frames))
        return torch.zeros(1)

    def frames_to_yuv(self, x, size=None, filter="bicubic", fmt="nv12", colour=None, frames=None, out=None, strides=None):
        self.calls.append(("frames_to_yuv", tuple(x.shape), size, filter, fmt, colour, frames))
        return torch.zeros(1)


def test_colour_none_is_the_old_call_and_a_colour_goes_to_frames_to_yuv(tmp_path):
    from tooncrafter_amd import ops, output
    from tooncrafter_amd.output import Colour
    spy, c = Spy(), Colour("bt709", "limited", "left")
    prev = ops.set_backend(spy)
    try:
        x = torch.zeros(1, 3, 4, 20, 32)
        output.clip_to_uint8(x)
        output.clip_to_uint8(x, True, colour=None)
        output.clip_to_uint8(x, True, (40, 64), "bicubic", "rgb24")               # the five positional arguments as before
        output.clip_to_uint8(x, fmt="nv12", filter="box", colour=None)
        output.clip_to_uint8(x, True, size=(40, 64), fmt="nv12", colour=c)
        output.clip_to_uint8(x, fmt="i420", filter="lanczos", colour=c)
        for bad in (dict(fmt="nv12", colour="bt709"), dict(fmt="nv12", colour=(1, 2))):
            with pytest.raises(ValueError):
                output.clip_to_uint8(x, **bad)
    finally:
        ops.set_backend(prev)
    assert spy.calls == [("video_to_uint8", (1, 3, 4, 20, 32)), ("video_to_uint8", (1, 3, 3, 20, 32)),
                         ("frames_to_u8", (1, 3, 4, 20, 32), (40, 64), "bicubic", "rgb24", (0, 3)),
                         ("frames_to_u8", (1, 3, 4, 20, 32), None, "box", "nv12", (0, 4)),
                         ("frames_to_yuv", (1, 3, 4, 20, 32), (40, 64), "bicubic", "nv12", c, (0, 3)),
                         ("frames_to_yuv", (1, 3, 4, 20, 32), None, "lanczos", "i420", c, (0, 4))]
    import inspect
    from tooncrafter_amd import clip, mp4
    for fn, name in ((output.clip_to_uint8, "colour"), (output.gather_frames, "colour"), (output.save_results_seperate, "colour"),
                     (output.planar_writer, "colour"), (mp4.write_mp4_i420, "colour"), (clip.synthesize_u8, "out_colour"),
                     (clip.synthesize_timeline_u8, "out_colour")):
        assert inspect.signature(fn).parameters[name].default is None, fn.__name__


def test_frames_to_yuv_rejects_what_a_colour_cannot_describe():
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.output import Colour
    from tooncrafter_amd.torch_ops import TorchLibOps
    x = torch.zeros(2, 3, 4, 20, 32)
    c8, c10 = Colour("bt709"), Colour("bt709", bits=10)
    for hip in (HipOps(), TorchLibOps()):
        for kw in (dict(fmt="rgb24", colour=c8), dict(fmt="p010", colour=c10), dict(fmt="i420", colour=c10), dict(colour=None),
                   dict(colour="bt709"), dict(colour=c8, size=(45, 72)), dict(colour=c10, size=(46, 71)), dict(colour=c8, filter="nearest"),
                   dict(colour=c8, frames=(0, 5)), dict(colour=c8, size=(0, 2))):
            with pytest.raises(ValueError):
                hip.frames_to_yuv(x, **kw)
        with pytest.raises(ValueError):
            hip.frames_to_yuv(x.double(), colour=c8)
        with pytest.raises(TooncrafterHipError):                                  # a well-formed CPU tensor: no fallback
            hip.frames_to_yuv(x, (46, 72), colour=c8)
        with pytest.raises(TooncrafterHipError):
            hip.frames_to_yuv(x, colour=c10, frames=(1, 2))
        for fmt in ("p010",):                                                     # and the old entry point keeps refusing the name
            with pytest.raises(ValueError):
                hip.frames_to_u8(x, fmt=fmt)


def test_save_results_writes_the_colour_into_the_file(tmp_path):
    """save_results_seperate(fmt="nv12", colour=) with the numpy statement standing in for the kernels"""
    from test_mp4_cpu import _decode
    from tooncrafter_amd import mp4, ops, output
    from tooncrafter_amd.output import Colour
    c = Colour("bt709", "limited", "left")

    class Statement:
        def frames_to_yuv(self, x, size=None, filter="bicubic", fmt="nv12", colour=None, frames=None, out=None, strides=None):
            rgb = ref.rgb_frames(x.numpy(), size, filter, colour.bits)[:, frames[0]:frames[0] + frames[1]]
            return torch.from_numpy(ref.packed(rgb, fmt, ref.out_matrix(colour.standard, colour.range, colour.bits), colour.siting))
    samples = torch.from_numpy(load_golden("pixel_back.npz")["x"])
    prev = ops.set_backend(Statement())
    try:
        written = output.save_results_seperate(["a prompt"], samples, "clip0.png", str(tmp_path / "samples"), fps=8, loop=True,
                                               size=(34, 50), filter="lanczos", fmt="nv12", colour=c)
    finally:
        ops.set_backend(prev)
    assert len(written) == 2
    rgb = ref.rgb_frames(samples.numpy(), (34, 50), "lanczos", 8)[:, :2]
    want = ref.packed(rgb, "i420", ref.out_matrix("bt709", "limited", 8), "left")
    for i, path in enumerate(written):
        plain = mp4.write_mp4_i420(str(tmp_path / f"plain{i}.mp4"), want[i], 50, 34, 8)      # the statement's planes, no colour
        d = _decode(plain)
        assert (d["w"], d["h"], len(d["frames"])) == (50, 34, 2)
        assert top_box(path, b"mdat") == top_box(plain, b"mdat")                  # the same samples
        vui = parse_sps(sps_of(path))["vui"]
        assert (vui["matrix_coefficients"], vui["video_full_range_flag"], vui["chroma_sample_loc_type_top_field"]) == (1, 0, 0)


def test_timeline_layout_with_a_colour():
    from tooncrafter_amd import clip
    from tooncrafter_amd.output import Colour
    old = clip.timeline_layout(3, 4, 1, (46, 72), "nv12")
    assert old == (7, 46 * 72 * 3 // 2, [(0, 1), (1, 1)])
    assert clip.timeline_layout(3, 4, 1, (46, 72), "nv12", None) == old
    assert clip.timeline_layout(3, 4, 1, (46, 72), "nv12", Colour("bt709")) == old
    assert clip.timeline_layout(3, 4, 1, (46, 72), "i420", Colour("bt709", siting="left")) == old
    assert clip.timeline_layout(4, 4, 2, (46, 72), "nv12", Colour(bits=10)) == (10, 46 * 72 * 3, [(0, 2), (2, 1)])
    for bad in (("rgb24", Colour()), ("i420", Colour(bits=10)), ("rgb24", Colour(bits=10))):
        with pytest.raises(ValueError):
            clip.timeline_layout(3, 4, 1, (46, 72), *bad)
    with pytest.raises(ValueError):
        clip.timeline_layout(3, 4, 1, (45, 72), "nv12", Colour())


def test_planes_from_frames_views_the_buffer():
    from tooncrafter_amd import clip
    from tooncrafter_amd.output import Colour
    h, w = 6, 8
    c8, c10 = Colour("bt709", "limited", "left"), Colour("bt709", "full", "center", 10)
    buf = torch.arange(2 * 3 * (h * w * 3 // 2), dtype=torch.int64).remainder(251).to(torch.uint8).view(2, 3, -1)
    for fmt in ("i420", "nv12"):
        p = clip.planes_from_frames(buf, h, w, fmt, c8)
        assert (p.fmt, p.standard, p.range, p.siting, p.matrix) == (fmt, "bt709", "limited", "left", None) and len(p) == 6
        assert p.y.shape == (6, h, w) and p.y.dtype == torch.uint8 and p.y.data_ptr() == buf.data_ptr()
        assert p.chroma[0].data_ptr() == buf.data_ptr() + h * w
        assert Colour.of(p) == c8
    last = clip.planes_from_frames(buf[:, -1], h, w, "nv12", c8)                  # a clip's last frames: the next keyframes
    assert len(last) == 2 and last.y.data_ptr() == buf[0, 2].data_ptr() and torch.equal(last.chroma[0][1].reshape(-1), buf[1, 2, h * w:])
    wide = torch.arange(2 * 3 * h * w * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(2, 3, -1)
    p = clip.planes_from_frames(wide, h, w, "nv12", c10)
    assert (p.fmt, p.standard, p.range, p.siting) == ("p010", "bt709", "full", "center") and Colour.of(p) == c10
    assert p.y.shape == (6, h, w) and p.y.element_size() == 2 and p.chroma[0].shape == (6, h // 2, w // 2, 2)
    assert p.y.data_ptr() == wide.data_ptr() and p.chroma[0].data_ptr() == wide.data_ptr() + 2 * h * w
    words = wide.numpy().reshape(6, -1).view("<u2")
    assert np.array_equal(p.y.view(torch.int16).numpy().view(np.uint16), words[:, :h * w].reshape(6, h, w))
    for bad in ((wide, h, w, "i420", c10), (wide, h, w, "nv12", c8), (buf, h, w, "nv12", c10), (buf, h, w, "rgb24", c8), (buf, h, w, "nv12", "bt709"),
                (buf, 5, w, "nv12", c8), (wide[..., 1:], h, w, "nv12", c10), (wide.to(torch.int16), h, w, "nv12", c10)):
        with pytest.raises(ValueError):
            clip.planes_from_frames(*bad)


def test_out_colour_source_needs_planes():
    from tooncrafter_amd import clip
    from tooncrafter_amd.output import Colour
    plan = clip.SamplingPlan(steps=2)
    rgb = torch.zeros(3, 20, 32, 3, dtype=torch.uint8)
    for bad in ("source", "bt709", 709):
        with pytest.raises(ValueError):
            clip.synthesize_timeline_u8(None, rgb, [1, 4, 4, 4, 4], size=(32, 32), plan=plan, out_fmt="nv12", out_colour=bad)
    with pytest.raises(ValueError):                                               # a colour describes planes
        clip.synthesize_timeline_u8(None, rgb, [1, 4, 4, 4, 4], size=(32, 32), plan=plan, out_fmt="rgb24", out_colour=Colour())
    with pytest.raises(ValueError):
        clip.synthesize_timeline_u8(None, rgb, [1, 4, 4, 4, 4], size=(32, 32), plan=plan, out_fmt="i420", out_colour=Colour(bits=10))


# ---------------------------------------------------------------- the writer says what the planes are

class BitReader:
    """H.264 7.2: u(n) and ue(v) over an RBSP (emulation prevention bytes already removed)"""
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(data, np.uint8))
        self.pos = 0

    def u(self, n):
        v = 0
        for b in self.bits[self.pos:self.pos + n]:
            v = (v << 1) | int(b)
        assert self.pos + n <= len(self.bits)
        self.pos += n
        return v

    def ue(self):
        zeros = 0
        while self.u(1) == 0:
            zeros += 1
        return (1 << zeros) - 1 + self.u(zeros)


def parse_sps(nal):
    """seq_parameter_set_data() of 7.3.2.1.1 for the profiles without chroma_format_idc (Baseline / Main / Extended) and
    vui_parameters() of E.1.1, written from the syntax tables; returns the fields read, `vui` None when absent"""
    assert nal[0] & 0x1F == 7
    rbsp = bytearray()
    zeros = 0
    for b in nal[1:]:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        rbsp.append(b)
        zeros = zeros + 1 if b == 0 else 0
    r = BitReader(bytes(rbsp))
    s = {"profile_idc": r.u(8), "constraints": r.u(8), "level_idc": r.u(8), "sps_id": r.ue()}
    assert s["profile_idc"] in (66, 77, 88)
    s["log2_max_frame_num_minus4"] = r.ue()
    s["pic_order_cnt_type"] = r.ue()
    assert s["pic_order_cnt_type"] == 2                                           # types 0 and 1 carry further fields
    s["max_num_ref_frames"], s["gaps"] = r.ue(), r.u(1)
    s["mbw"], s["mbh"] = r.ue() + 1, r.ue() + 1
    s["frame_mbs_only_flag"] = r.u(1)
    assert s["frame_mbs_only_flag"] == 1                                          # else mb_adaptive_frame_field_flag follows
    s["direct_8x8_inference_flag"] = r.u(1)
    s["crop"] = [r.ue() for _ in range(4)] if r.u(1) else None
    s["vui"] = None
    if r.u(1):
        v = s["vui"] = {}
        v["aspect_ratio_info_present_flag"] = r.u(1)
        assert not v["aspect_ratio_info_present_flag"]
        v["overscan_info_present_flag"] = r.u(1)
        assert not v["overscan_info_present_flag"]
        v["video_signal_type_present_flag"] = r.u(1)
        if v["video_signal_type_present_flag"]:
            v["video_format"], v["video_full_range_flag"] = r.u(3), r.u(1)
            v["colour_description_present_flag"] = r.u(1)
            if v["colour_description_present_flag"]:
                v["colour_primaries"], v["transfer_characteristics"], v["matrix_coefficients"] = r.u(8), r.u(8), r.u(8)
        v["chroma_loc_info_present_flag"] = r.u(1)
        if v["chroma_loc_info_present_flag"]:
            v["chroma_sample_loc_type_top_field"], v["chroma_sample_loc_type_bottom_field"] = r.ue(), r.ue()
        for flag in ("timing_info_present_flag", "nal_hrd_parameters_present_flag", "vcl_hrd_parameters_present_flag",
                     "pic_struct_present_flag", "bitstream_restriction_flag"):
            v[flag] = r.u(1)
            assert not v[flag], flag                                              # each would carry further fields
    assert r.u(1) == 1 and not r.bits[r.pos:].any() and len(r.bits) - r.pos < 8   # rbsp_trailing_bits end the unit
    return s


def sps_of(path):
    """the one SPS NAL unit of the avcC box (ISO/IEC 14496-15 5.2.4.1)"""
    data = open(path, "rb").read()
    at = data.index(b"avcC") + 4
    assert data[at] == 1 and data[at + 5] & 0x1F == 1
    n = struct.unpack(">H", data[at + 6:at + 8])[0]
    return data[at + 8:at + 8 + n]


def top_box(path, kind):
    """the payload of the file's top-level box `kind`"""
    data = open(path, "rb").read()
    at = 0
    while at < len(data):
        size, name = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if name == kind:
            return data[at + 8:at + size]
        at += size
    raise AssertionError(f"no {kind!r} box")


@pytest.mark.parametrize("colour,codes,full,loc", [(("bt709", "limited", "left"), 1, 0, 0), (("bt601", "full", "center"), 6, 1, 1)])
def test_mp4_carries_the_colour(tmp_path, colour, codes, full, loc):
    from tooncrafter_amd import mp4, output
    from tooncrafter_amd.output import Colour
    c = Colour(*colour)
    rng = np.random.default_rng(7400)
    t, h, w = 2, 34, 50
    planes = rng.integers(0, 256, (t, h * w * 3 // 2), dtype=np.uint8)
    plain = mp4.write_mp4_i420(str(tmp_path / "plain.mp4"), planes, w, h, fps=8)
    assert open(mp4.write_mp4_i420(str(tmp_path / "none.mp4"), planes, w, h, 8, colour=None), "rb").read() == open(plain, "rb").read()
    s = parse_sps(sps_of(plain))                                                  # the reader on the default stream: no VUI
    assert s["vui"] is None and (s["mbw"], s["mbh"]) == (4, 3) and s["crop"] == [0, 7, 0, 7] and s["profile_idc"] == 66
    assert b"colr" not in open(plain, "rb").read()
    path = mp4.write_mp4_i420(str(tmp_path / "colour.mp4"), planes, w, h, fps=8, colour=c)
    s2 = parse_sps(sps_of(path))
    assert {k: v for k, v in s2.items() if k != "vui"} == {k: v for k, v in s.items() if k != "vui"}
    assert s2["vui"] == {
        "aspect_ratio_info_present_flag": 0, "overscan_info_present_flag": 0, "video_signal_type_present_flag": 1, "video_format": 5,
        "video_full_range_flag": full, "colour_description_present_flag": 1, "colour_primaries": codes,
        "transfer_characteristics": codes, "matrix_coefficients": codes, "chroma_loc_info_present_flag": 1,
        "chroma_sample_loc_type_top_field": loc, "chroma_sample_loc_type_bottom_field": loc, "timing_info_present_flag": 0,
        "nal_hrd_parameters_present_flag": 0, "vcl_hrd_parameters_present_flag": 0, "pic_struct_present_flag": 0,
        "bitstream_restriction_flag": 0}
    data = open(path, "rb").read()
    box = struct.pack(">I", 19) + b"colr" + b"nclx" + struct.pack(">HHHB", codes, codes, codes, full << 7)
    assert data.count(box) == 1 and data.count(b"colr") == 1
    at = data.index(b"avc1", data.index(b"stsd")) - 4                             # the box sits at the end of the avc1 sample entry
    assert data.index(box) + 19 == at + struct.unpack(">I", data[at:at + 4])[0]
    # the samples are the same: only the SPS and the colr box were added
    assert top_box(path, b"mdat") == top_box(plain, b"mdat") and len(top_box(path, b"mdat")) > t * h * w * 3 // 2
    # NV12 through planar_writer(colour=): the same file
    n = h * w
    nv12 = planes.copy()
    nv12[:, n::2], nv12[:, n + 1::2] = planes[:, n:n + n // 4], planes[:, n + n // 4:]
    other = output.planar_writer(w, h, "nv12", colour=c)(str(tmp_path / "nv12.mp4"), torch.from_numpy(nv12), 8)
    assert open(other, "rb").read() == data
    for bad in (Colour(bits=10), "bt709"):
        with pytest.raises(ValueError):
            mp4.write_mp4_i420(str(tmp_path / "bad.mp4"), planes, w, h, 8, colour=bad)
