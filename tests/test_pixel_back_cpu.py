"""The pixel back end without a GPU (tc_resize_tables_filter, tc_frames_to_u8; additive within ABI 14): the entry points are
declared, exported and bound with the header's struct layout; the host table builder equals the numpy statement of
tests/pixel_back_ref.py for PIL's four filters, and that statement equals PIL; the integer BT.601 conversion has its reference
points and stays within one code value of mp4.rgb_to_yuv420; every documented refusal returns before any device call; the
Meta-key operator infers shapes; the Python interface rejects wrong dtypes and layouts; write_mp4_i420 stores its planes and
write_mp4 its old bytes; the committed fixture is what its generator writes.  Compute is covered by
tests/test_gpu_pixel_back.py."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import pixel_back_ref as ref
from conftest import GOLDEN, ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
OUT_FIELDS = ("x", "out", "b", "t", "h", "w", "f0", "nf", "oh", "ow", "format", "pitch", "frame_stride", "clip_stride",
              "h_bounds", "h_coefs", "h_kmax", "v_bounds", "v_coefs", "v_kmax", "workspace", "workspace_bytes")
ENTRY_POINTS = ("tc_resize_tables_filter", "tc_frames_to_u8_workspace", "tc_frames_to_u8")
# source (h, w) -> the (oh, ow) on which the statement was checked against Pillow 12.2 (hard 0 / 255 edges: overshoot clips)
PIL_SIZES = [((20, 32), [(40, 64), (45, 72), (10, 16), (14, 22), (20, 50), (33, 32), (7, 5)]),
             ((40, 64), [(136, 240)]), ((6, 8), [(48, 64)])]
# write_mp4 of the frame set below at the commit before encode_h264_ipcm was factored: the file's bytes must not move
WRITE_MP4_SHA256 = "e478f076b9db605628a7211ce95b68c7156614f579b2c565c1790bf4b9f0dd42"
I32P = ctypes.POINTER(ctypes.c_int32)


def c_tables(lib, code, n_in, n_out):
    kmax = lib.tc_resize_tables_filter(code, n_in, n_out, None, None, 0)
    assert kmax > 0
    bounds, coefs = np.full((n_out, 2), -7, np.int32), np.full((n_out, kmax), -7, np.int32)
    assert lib.tc_resize_tables_filter(code, n_in, n_out, bounds.ctypes.data_as(I32P), coefs.ctypes.data_as(I32P), coefs.size) == kmax
    return bounds, coefs


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_the_entry_points_and_abi_is_unchanged():
    from tooncrafter_amd import _lib
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"#define\s+TC_ABI_VERSION\s+14\b", header) and _lib.TC_ABI_VERSION == 14
    assert re.search(r"\bint32_t\s+tc_resize_tables_filter\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", header)
    assert re.search(r"\bint\s+tc_frames_to_u8\s*\(\s*const\s+TcFramesOutParams\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"\bint64_t\s+tc_frames_to_u8_workspace\s*\(\s*const\s+TcFramesOutParams\s*\*\s*\w+\s*\)\s*;", header)
    for i, name in enumerate(ref.FILTERS):
        assert re.search(rf"\bTC_RESIZE_{name.upper()}\s*=\s*{i}\b", header) and _lib.TC_RESIZE_FILTERS[name] == i
    for i, name in enumerate(ref.FORMATS):
        assert re.search(rf"\bTC_PIXFMT_{name.upper()}\s*=\s*{i}\b", header) and _lib.TC_PIXFMTS[name] == i
    doc = header[header.index("Pixel back end"):header.index("int tc_frames_to_u8(")]
    for word in ("inference.py:146-155", "16829", "33039", "6416", "-9714", "19070", "28784", "24103", "4681", "reciprocal",
                 "TC_EINVAL", "TC_ESHAPE", "TC_EWORKSPACE", "clip_stride", "rgb_to_yuv420"):
        assert word in doc, word
    # tc_resize_tables itself is as it was
    assert "int32_t tc_resize_tables(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs, int64_t coefs_len);" in header


def test_ctypes_struct_matches_the_compiled_header(tmp_path):
    """A probe compiled against the header prints sizeof and every offsetof; the ctypes mirror must agree."""
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcFramesOutParams._fields_) == OUT_FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %zu", TC_ABI_VERSION, sizeof(TcFramesOutParams));']
    lines += [f'  printf(" %zu", offsetof(TcFramesOutParams, {f}));' for f in OUT_FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [14, ctypes.sizeof(_lib.TcFramesOutParams)]
    assert got[2:] == [getattr(_lib.TcFramesOutParams, f).offset for f in OUT_FIELDS]


def test_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_frames_to_u8"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcFramesOutParams), ctypes.c_void_p])
    assert _lib.SYMBOLS["tc_frames_to_u8_workspace"] == (ctypes.c_int64, [ctypes.POINTER(_lib.TcFramesOutParams)])
    assert _lib.load().tc_abi_version() == 14
    assert "pixel_back.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pixel_back.hip"))
    from tooncrafter_amd import clip, mp4, output
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    assert callable(HipOps.frames_to_u8) and TorchLibOps.frames_to_u8 is not HipOps.frames_to_u8
    assert callable(mp4.encode_h264_ipcm_yuv) and callable(mp4.write_mp4_i420) and callable(output.planar_writer)
    import inspect
    for fn, names in ((output.clip_to_uint8, ("size", "filter", "fmt")), (output.gather_frames, ("size", "filter", "fmt")),
                      (output.save_results_seperate, ("size", "filter", "fmt")), (clip.synthesize_u8, ("out_size", "out_filter", "out_fmt"))):
        params = inspect.signature(fn).parameters
        assert [params[n].default for n in names] == [None, "bicubic", "rgb24"], fn.__name__


# ---------------------------------------------------------------- the table builder and its statement

@pytest.mark.parametrize("name", ref.FILTERS)
def test_filter_tables_equal_the_numpy_statement(name):
    """Bounds and every coefficient, over in, out in 1 .. 48 and three frame sizes; the columns of a row past its tap count
    are zero (the statement's are)."""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    code = ref.FILTERS.index(name)
    pairs = [(i, o) for i in range(1, 49) for o in range(1, 49)] + [(320, 640), (512, 1024), (320, 180)]
    negative = False
    for n_in, n_out in pairs:
        bounds, coefs = c_tables(lib, code, n_in, n_out)
        want_b, want_c = ref.tables(name, n_in, n_out)
        assert coefs.shape == want_c.shape, (n_in, n_out)
        assert np.array_equal(bounds, want_b) and np.array_equal(coefs, want_c), (n_in, n_out)
        negative = negative or bool((coefs < 0).any())
    assert negative == (name in ("bicubic", "lanczos"))                           # the lobes the -0.5 rounding is for
    want_kmax = {"bilinear": 5, "bicubic": 9, "lanczos": 13, "box": 3}[name]      # 320 -> 180: fs = 16 / 9
    assert lib.tc_resize_tables_filter(code, 320, 180, None, None, 0) == want_kmax


def test_bilinear_tables_are_tc_resize_tables():
    """every size pair 1 .. 128 both ways: the range tc_resize_tables' comment claims for the two forms of the weight"""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    for n_in in range(1, 129):
        for n_out in range(1, 129):
            bounds, coefs = c_tables(lib, 0, n_in, n_out)
            kmax = lib.tc_resize_tables(n_in, n_out, None, None, 0)
            assert kmax == coefs.shape[1], (n_in, n_out)
            old_b, old_c = np.full((n_out, 2), -7, np.int32), np.full((n_out, kmax), -7, np.int32)
            assert lib.tc_resize_tables(n_in, n_out, old_b.ctypes.data_as(I32P), old_c.ctypes.data_as(I32P), old_c.size) == kmax
            assert np.array_equal(bounds, old_b) and np.array_equal(coefs, old_c), (n_in, n_out)


def test_resize_tables_filter_refuses_bad_arguments():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    buf = np.full(256, -7, np.int32)
    ptr = buf.ctypes.data_as(I32P)
    f = lib.tc_resize_tables_filter
    assert f(4, 8, 4, None, None, 0) == -1 and f(-1, 8, 4, None, None, 0) == -1                    # unknown filter
    for code in range(4):
        assert f(code, 0, 4, None, None, 0) == -1 and f(code, 4, -1, None, None, 0) == -1
        assert f(code, 8, 4, ptr, None, 256) == -1 and f(code, 8, 4, None, ptr, 256) == -1
        kmax = f(code, 8, 4, None, None, 0)
        assert kmax == {0: 5, 1: 9, 2: 13, 3: 3}[code]
        assert f(code, 8, 4, ptr, ptr, 4 * kmax - 1) == -4
    assert (buf == -7).all()


def test_the_statement_equals_pil():
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for i, ((h, w), sizes) in enumerate(PIL_SIZES):
        rng = np.random.default_rng(7200 + i)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[h // 4:h // 2, w // 4:w // 2] = 255                                    # hard edges: the overshoot must clip
        img[h // 2:3 * h // 4, w // 8:w // 2] = 0
        img[:, 3 * w // 4] = (255, 0, 255)
        for oh, ow in sizes:
            for name in ref.FILTERS:
                want = np.asarray(Image.fromarray(img).resize((ow, oh), getattr(Image, name.upper())))
                assert np.array_equal(ref.resize(img, oh, ow, name), want), ((h, w), (oh, ow), name)
                n += 1
    assert n == 36


# ---------------------------------------------------------------- the integer colour conversion

def test_integer_yuv_reference_points_and_distance_to_the_float_expression():
    from tooncrafter_amd import mp4
    px = np.array([[[0, 0, 0], [255, 255, 255]], [[255, 0, 0], [0, 0, 255]]], dtype=np.uint8)
    y, cb, cr = ref.yuv420(px)
    assert y.tolist() == [[16, 235], [81, 41]] and cb.tolist() == [[147]] and cr.tolist() == [[151]]
    assert 16829 + 33039 + 6416 == 56284 and -9714 - 19070 + 28784 == 0 and 28784 - 24103 - 4681 == 0
    # 40 random 64 x 96 frames and a 52^3 colour grid (every colour of the grid in 2 x 2 blocks of mixed neighbours)
    rng = np.random.default_rng(7300)
    frames = list(rng.integers(0, 256, (40, 64, 96, 3), dtype=np.uint8))
    lv = np.linspace(0, 255, 52).round().astype(np.uint8)
    grid = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(52 * 26, 104, 3)
    frames.append(grid)
    worst, diff_y, diff_c, n_y, n_c = 0, 0, 0, 0, 0
    for f in frames:
        a, b = ref.yuv420(f), mp4.rgb_to_yuv420(f)
        d = [np.abs(u.astype(np.int32) - v.astype(np.int32)) for u, v in zip(a, b)]
        worst = max(worst, *(int(v.max()) for v in d))
        diff_y, n_y = diff_y + int((d[0] != 0).sum()), n_y + d[0].size
        diff_c, n_c = diff_c + int((d[1] != 0).sum() + (d[2] != 0).sum()), n_c + d[1].size + d[2].size
    print(f"integer vs float32 BT.601: Y {diff_y}/{n_y} differ, chroma {diff_c}/{n_c} differ, worst {worst}")
    assert worst <= 1


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_frames_to_u8_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    x = (ctypes.c_float * (2 * 3 * 3 * 20 * 32))()
    out = (ctypes.c_uint8 * (2 * 3 * 46 * 72 * 3))()
    tab = (ctypes.c_int32 * 1024)()
    ws = (ctypes.c_uint8 * 64)()

    def params(**kw):
        p = _lib.TcFramesOutParams(x=ctypes.addressof(x), out=ctypes.addressof(out), b=2, t=3, h=20, w=32, f0=0, nf=3, oh=46, ow=72,
                                   format=0, pitch=216, frame_stride=46 * 216, clip_stride=3 * 46 * 216, h_kmax=5, v_kmax=5)
        p.h_bounds = p.h_coefs = p.v_bounds = p.v_coefs = ctypes.addressof(tab)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rc(**kw):
        return lib.tc_frames_to_u8(ctypes.byref(params(**kw)), None)
    yuv = dict(format=1, pitch=72, frame_stride=46 * 72 * 3 // 2, clip_stride=3 * 46 * 72 * 3 // 2)
    assert lib.tc_frames_to_u8(None, None) == -1 and lib.tc_frames_to_u8_workspace(None) == 0
    assert rc(x=None) == -1 and rc(out=None) == -1
    for name in ("b", "t", "h", "w", "oh", "ow"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -2}) == -1, name
    assert rc(f0=-1) == -1 and rc(nf=0) == -1 and rc(f0=1) == -1 and rc(f0=3, nf=1) == -1 and rc(nf=4) == -1      # outside the clip
    assert rc(format=3) == -1 and rc(format=-1) == -1
    assert rc(pitch=215) == -1 and rc(**dict(yuv, pitch=70)) == -1                # a row does not hold its pixels
    assert rc(frame_stride=46 * 216 - 1) == -1 and rc(**dict(yuv, frame_stride=46 * 72 * 3 // 2 - 1)) == -1
    assert rc(**dict(yuv, format=2, frame_stride=46 * 72 * 3 // 2 - 1)) == -1
    assert rc(clip_stride=3 * 46 * 216 - 1) == -1                                 # clips overlap ...
    assert rc(b=1, clip_stride=0) == -4                                           # ... which one clip cannot (on to the workspace)
    assert rc(h_coefs=None) == -1 and rc(h_bounds=None) == -1 and rc(v_bounds=None) == -1 and rc(v_coefs=None) == -1
    assert rc(h_kmax=0) == -1 and rc(v_kmax=-1) == -1                             # resampled, but a table is missing
    assert rc(oh=20, v_bounds=None, v_coefs=None, v_kmax=0, frame_stride=20 * 216, clip_stride=3 * 20 * 216) == -4      # not of a pass that is skipped
    # odd sizes in the planar formats
    for fmt in (1, 2):
        assert rc(**dict(yuv, format=fmt, oh=45)) == -3 and rc(**dict(yuv, format=fmt, ow=71)) == -3
    assert rc(**dict(yuv, pitch=73)) == -3 and rc(**dict(yuv, format=2, pitch=73, frame_stride=46 * 73 * 3 // 2 + 73,
                                                         clip_stride=3 * (46 * 73 * 3 // 2 + 73))) == -4        # NV12 takes an odd pitch
    # workspace: the uint8 frames at source size + the horizontal intermediate when ow != w; nothing for identity RGB24
    n = 2 * 3
    assert lib.tc_frames_to_u8_workspace(ctypes.byref(params())) == n * 20 * 32 * 3 + n * 20 * 72 * 3
    assert lib.tc_frames_to_u8_workspace(ctypes.byref(params(f0=1, nf=2, clip_stride=2 * 46 * 216))) == 4 * (20 * 32 * 3 + 20 * 72 * 3)
    vonly = dict(ow=32, pitch=96, frame_stride=46 * 96, clip_stride=3 * 46 * 96)
    assert lib.tc_frames_to_u8_workspace(ctypes.byref(params(**vonly))) == n * 20 * 32 * 3
    ident = dict(oh=20, ow=32, pitch=96, frame_stride=20 * 96, clip_stride=3 * 20 * 96)
    assert lib.tc_frames_to_u8_workspace(ctypes.byref(params(**ident))) == 0
    ident_yuv = dict(oh=20, ow=32, format=1, pitch=32, frame_stride=960, clip_stride=3 * 960)
    assert lib.tc_frames_to_u8_workspace(ctypes.byref(params(**ident_yuv))) == n * 20 * 32 * 3
    assert lib.tc_frames_to_u8_workspace(ctypes.byref(params(format=7))) == 0     # a refused request needs none
    need = n * 20 * 32 * 3 + n * 20 * 72 * 3
    assert rc(workspace=None, workspace_bytes=1 << 30) == -4
    assert rc(workspace=ctypes.addressof(ws), workspace_bytes=need - 1) == -4
    assert rc(**dict(ident_yuv, workspace=ctypes.addressof(ws), workspace_bytes=n * 20 * 32 * 3 - 1)) == -4
    assert not any(out) and not any(tab) and not any(ws)


# ---------------------------------------------------------------- the operator layer and the Python interface

def test_meta_kernel_infers_shape_and_dtype():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    assert str(t.frames_to_u8.default._schema).startswith("tooncrafter::frames_to_u8(Tensor x, int oh, int ow, int format, int f0, int nf,")
    x = torch.empty(2, 3, 5, 20, 32, device="meta")
    def tabs(n_out):                                      # the tables of one resized axis: a row per output index
        return torch.empty(n_out, 2, dtype=torch.int32, device="meta"), torch.empty(n_out, 4, dtype=torch.int32, device="meta")
    up = tabs(72) + tabs(46)                              # (20, 32) -> (46, 72): w -> ow, then h -> oh
    y = t.frames_to_u8(x, 46, 72, 0, 0, 5, *up)
    assert y.shape == (2, 5, 46, 72, 3) and y.dtype == torch.uint8 and y.device.type == "meta"
    for fmt in (1, 2):
        y = t.frames_to_u8(x, 46, 72, fmt, 1, 3, *up)
        assert y.shape == (2, 3, 46 * 72 * 3 // 2) and y.dtype == torch.uint8 and y.device.type == "meta"
    y = t.frames_to_u8(x, 46, 32, 0, 0, 5, None, None, *tabs(46))                # None for the axis that keeps its size
    assert y.shape == (2, 5, 46, 32, 3) and y.dtype == torch.uint8 and y.device.type == "meta"
    assert t.frames_to_u8(x, 20, 32, 0, 4, 1, None, None, None, None).shape == (2, 1, 20, 32, 3)
    for tables in ((None,) * 4, tabs(4) * 2, tabs(46) + tabs(72)):                # a resize without its tables: refused as on the CUDA key
        with pytest.raises(RuntimeError, match="tables of"):
            t.frames_to_u8(x, 46, 72, 0, 0, 5, *tables)
    for bad in ((45, 72, 1, 0, 5), (46, 71, 2, 0, 5), (46, 72, 3, 0, 5), (46, 72, 0, 3, 3), (46, 72, 0, 0, 0), (0, 72, 0, 0, 5)):
        with pytest.raises(RuntimeError):
            t.frames_to_u8(x, *bad, None, None, None, None)
    with pytest.raises((RuntimeError, NotImplementedError)):                      # no CPU kernel is registered: no fallback
        t.frames_to_u8(torch.zeros(1, 3, 2, 20, 32), 20, 32, 0, 0, 2, None, None, None, None)


def test_python_interface_rejects_wrong_dtypes_and_layouts():
    from tooncrafter_amd import output
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    x = torch.zeros(2, 3, 4, 20, 32)
    for hip in (HipOps(), TorchLibOps()):
        for bad in (x.double(), x.to(torch.uint8), x[0], x[:, :2], x[:, :, :0], "clip"):
            with pytest.raises(ValueError):
                hip.frames_to_u8(bad, (46, 72))
        for kw in (dict(size=(0, 72)), dict(size=(46, -1)), dict(filter="nearest"), dict(fmt="yuv444"), dict(frames=(0, 5)),
                   dict(frames=(-1, 2)), dict(frames=(2, 0)), dict(frames=(4, 1)), dict(size=(45, 72), fmt="i420"),
                   dict(size=(46, 71), fmt="nv12"), dict(size=(21, 32), fmt="i420")):
            with pytest.raises(ValueError):
                hip.frames_to_u8(x, **kw)
        with pytest.raises(TooncrafterHipError):                                  # a well-formed CPU tensor: no fallback
            hip.frames_to_u8(x, (46, 72))
        with pytest.raises(TooncrafterHipError):
            hip.frames_to_u8(x, fmt="i420", frames=(1, 2))
    with pytest.raises(ValueError):
        output.clip_to_uint8(x, size=(45, 72), fmt="i420")


def test_clip_to_uint8_without_the_new_keywords_is_the_old_call():
    """(samples, loop) alone goes to ops.video_to_uint8 with the sliced clip, as before; a size or a planar format goes to
    ops.frames_to_u8 with `loop` as a frame count."""
    from tooncrafter_amd import ops, output

    class Spy:
        def __init__(self):
            self.calls = []

        def video_to_uint8(self, video):
            self.calls.append(("video_to_uint8", tuple(video.shape)))
            return "old"

        def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
            self.calls.append(("frames_to_u8", tuple(x.shape), size, filter, fmt, frames))
            return "new"
    spy = Spy()
    prev = ops.set_backend(spy)
    try:
        x = torch.zeros(1, 3, 4, 20, 32)
        assert output.clip_to_uint8(x) == "old" and output.clip_to_uint8(x, True) == "old" and output.clip_to_uint8(x, loop=True) == "old"
        assert output.clip_to_uint8(x, True, size=(40, 64)) == "new"
        assert output.clip_to_uint8(x, fmt="nv12", filter="box") == "new"
    finally:
        ops.set_backend(prev)
    assert spy.calls == [("video_to_uint8", (1, 3, 4, 20, 32)), ("video_to_uint8", (1, 3, 3, 20, 32)), ("video_to_uint8", (1, 3, 3, 20, 32)),
                         ("frames_to_u8", (1, 3, 4, 20, 32), (40, 64), "bicubic", "rgb24", (0, 3)),
                         ("frames_to_u8", (1, 3, 4, 20, 32), None, "box", "nv12", (0, 4))]


# ---------------------------------------------------------------- the writer

def test_write_mp4_i420_stores_its_planes(tmp_path):
    from test_mp4_cpu import _decode
    from tooncrafter_amd import mp4, output
    rng = np.random.default_rng(7400)
    t, h, w = 3, 34, 50                                                           # not whole macroblocks: padded and cropped
    planes = rng.integers(0, 256, (t, h * w * 3 // 2), dtype=np.uint8)
    planes[0, :64] = 0                                                            # runs of zero bytes: emulation prevention
    path = mp4.write_mp4_i420(str(tmp_path / "clip.mp4"), torch.from_numpy(planes), w, h, fps=8)
    d = _decode(path)
    assert (d["w"], d["h"]) == (w, h) and abs(d["fps"] - 8.0) < 1e-9 and len(d["frames"]) == t
    n = h * w
    for i in range(t):
        y, cb, cr = d["frames"][i]
        assert np.array_equal(y.ravel(), planes[i, :n]) and np.array_equal(cb.ravel(), planes[i, n:n + n // 4])
        assert np.array_equal(cr.ravel(), planes[i, n + n // 4:])
    # NV12 planes through output.planar_writer: the same file
    nv12 = planes.copy()
    nv12[:, n::2], nv12[:, n + 1::2] = planes[:, n:n + n // 4], planes[:, n + n // 4:]
    other = output.planar_writer(w, h, "nv12")(str(tmp_path / "nv12.mp4"), torch.from_numpy(nv12), 8)
    assert open(other, "rb").read() == open(path, "rb").read()
    # the integer conversion of RGB frames, through the plane writer, decodes to those planes
    frames = rng.integers(0, 256, (2, 32, 48, 3), dtype=np.uint8)
    d = _decode(mp4.write_mp4_i420(str(tmp_path / "rgb.mp4"), ref.packed(frames, "i420"), 48, 32, fps=8))
    for i in range(2):
        assert all(np.array_equal(a, b) for a, b in zip(d["frames"][i], ref.yuv420(frames[i])))
    for bad in ((planes[:, :-1], w, h), (planes, w + 2, h), (planes.astype(np.int16), w, h), (planes, 25, 68)):
        with pytest.raises(ValueError):
            mp4.write_mp4_i420(str(tmp_path / "bad.mp4"), *bad)


def test_save_results_hands_planar_frames_to_the_plane_writer(tmp_path):
    """save_results_seperate(size=, fmt="nv12") with the numpy statement standing in for the kernels: the file holds the
    statement's planes of the resized frames, `loop` dropped the last one."""
    from test_mp4_cpu import _decode
    from tooncrafter_amd import ops, output

    class Statement:
        def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
            rgb = ref.resize(ref.to_u8(x.numpy())[:, frames[0]:frames[0] + frames[1]], size[0], size[1], filter)
            return torch.from_numpy(ref.packed(rgb, fmt))
    samples = torch.from_numpy(load_golden("pixel_back.npz")["x"])
    prev = ops.set_backend(Statement())
    try:
        written = output.save_results_seperate(["a prompt"], samples, "clip0.png", str(tmp_path / "samples"), fps=8, loop=True,
                                               size=(34, 50), filter="lanczos", fmt="nv12")
    finally:
        ops.set_backend(prev)
    assert [os.path.basename(p) for p in written] == ["clip0_sample0.mp4", "clip0_sample1.mp4"]
    rgb = ref.resize(ref.to_u8(samples.numpy()), 34, 50, "lanczos")
    for i, path in enumerate(written):
        d = _decode(path)
        assert (d["w"], d["h"], len(d["frames"])) == (50, 34, 2)
        for j in range(2):
            assert all(np.array_equal(a, b) for a, b in zip(d["frames"][j], ref.yuv420(rgb[i, j])))


def test_write_mp4_keeps_its_bytes(tmp_path):
    from tooncrafter_amd import mp4
    frames = np.random.default_rng(20261020).integers(0, 256, size=(3, 34, 50, 3), dtype=np.uint8)
    path = mp4.write_mp4(str(tmp_path / "a.mp4"), frames, fps=8)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == WRITE_MP4_SHA256
    sps, pps, slices = mp4.encode_h264_ipcm(frames)
    planes = [mp4.rgb_to_yuv420(f) for f in frames]
    assert (sps, pps, slices) == mp4.encode_h264_ipcm_yuv(*(np.stack([p[k] for p in planes]) for k in range(3)))


# ---------------------------------------------------------------- the fixture

def test_pixel_back_fixture_is_what_the_generator_writes(tmp_path):
    pytest.importorskip("PIL.Image")
    out = tmp_path / "pixel_back.npz"
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_pixel_back_golden.py"), "--out", str(out)], check=True,
                   capture_output=True, env=env, timeout=300)
    new, old = dict(np.load(out)), load_golden("pixel_back.npz")
    assert sorted(new) == sorted(old) and len(old) == 1 + 4 * 4
    for k in sorted(old):
        assert new[k].shape == old[k].shape and new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k
    assert old["x"].shape == (2, 3, 3, 20, 32) and old["x"].dtype == np.float32 and old["x"].min() < -1 and old["x"].max() > 1
    assert os.path.getsize(os.path.join(GOLDEN, "pixel_back.npz")) < 300 * 1024


def test_the_statement_reproduces_the_fixture():
    """what the GPU tests rely on: the fixture's PIL frames are the statement's resize of the statement's uint8 frames"""
    g = load_golden("pixel_back.npz")
    u8 = ref.to_u8(g["x"])
    for k in sorted(g):
        if k != "x":
            name, size = k.split(".")
            oh, ow = (int(v) for v in size.split("x"))
            assert np.array_equal(ref.resize(u8, oh, ow, name), g[k]), k
