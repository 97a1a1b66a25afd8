"""The pixel front end without a GPU (tc_resize_tables, tc_frames_from_u8, tc_clip_patches; additive within ABI 14): the entry
points are declared, exported and bound with the header's struct layout; the host table builder equals a numpy statement of
PIL's 8-bit BILINEAR coefficients, and that statement equals PIL; every documented refusal returns before any device call;
the Meta-key operators infer shapes; the Python interface rejects wrong dtypes and layouts; the committed fixture is what
its generator writes.  Compute is covered by tests/test_gpu_pixel_front.py."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
FRAMES_FIELDS = ("src", "image_stride", "pitch", "n", "sh", "sw", "slots", "out", "b", "t", "h", "w", "h_bounds", "h_coefs",
                 "h_kmax", "v_bounds", "v_coefs", "v_kmax", "workspace", "workspace_bytes")
CLIP_FIELDS = ("x", "out", "b", "h", "w", "size", "patch", "ld", "antialias", "mean", "std", "workspace", "workspace_bytes")
ENTRY_POINTS = ("tc_resize_tables", "tc_frames_from_u8_resized", "tc_frames_from_u8_workspace", "tc_frames_from_u8",
                "tc_clip_patches_workspace", "tc_clip_patches")
# (h, w) -> (h, w) pairs on which the statement below was checked against PIL
PIL_PAIRS = [((37, 53), (20, 29)), ((64, 64), (32, 32)), ((100, 150), (320, 480)), ((333, 517), (320, 497)),
             ((720, 1280), (320, 569)), ((1080, 1920), (320, 569)), ((17, 9), (16, 9)), ((48, 80), (47, 80)), ((5, 7), (11, 3))]


# ---------------------------------------------------------------- the numpy statement of PIL's 8-bit BILINEAR resample

def pil_tables(n_in, n_out):
    """(bounds [n_out, 2] = (xmin, count), coefs [n_out, kmax]) int32 of one axis n_in -> n_out: Pillow's precompute_coeffs
    and normalize_coeffs_8bpc for the bilinear filter, in Python floats (IEEE doubles), weights summed in tap order."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    kmax = int(math.ceil(support)) * 2 + 1
    bounds, coefs = np.zeros((n_out, 2), np.int32), np.zeros((n_out, kmax), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            v = v / total if total != 0.0 else v
            coefs[xx, x] = int(v * (1 << 22) + (0.5 if v >= 0 else -0.5))
        bounds[xx] = (xmin, xmax - xmin)
    return bounds, coefs


def pil_pass(img, n_out, axis):
    """one pass over `axis` of a uint8 array: clip(((1 << 21) + sum k * src) >> 22, 0, 255)"""
    bounds, coefs = pil_tables(img.shape[axis], n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.int64)
    for xx, (xmin, cnt) in enumerate(bounds):
        acc = np.tensordot(coefs[xx, :cnt].astype(np.int64), src[xmin:xmin + cnt], axes=1)
        out[xx] = np.clip(((1 << 21) + acc) >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def pil_resize(img, oh, ow):
    """(h, w, c) uint8 -> (oh, ow, c): horizontal pass, then vertical; a pass whose size does not change is skipped"""
    if img.shape[1] != ow:
        img = pil_pass(img, ow, 1)
    if img.shape[0] != oh:
        img = pil_pass(img, oh, 0)
    return img


def c_tables(lib, n_in, n_out):
    i32p = ctypes.POINTER(ctypes.c_int32)
    kmax = lib.tc_resize_tables(n_in, n_out, None, None, 0)
    assert kmax > 0
    bounds, coefs = np.full((n_out, 2), -7, np.int32), np.full((n_out, kmax), -7, np.int32)
    assert lib.tc_resize_tables(n_in, n_out, bounds.ctypes.data_as(i32p), coefs.ctypes.data_as(i32p), coefs.size) == kmax
    return bounds, coefs


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_the_entry_points_and_abi_is_unchanged():
    from tooncrafter_amd import _lib
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"#define\s+TC_ABI_VERSION\s+14\b", header) and _lib.TC_ABI_VERSION == 14
    assert re.search(r"\bint32_t\s+tc_resize_tables\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", header)
    assert re.search(r"\bint\s+tc_frames_from_u8\s*\(\s*const\s+TcFramesU8Params\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"\bint\s+tc_clip_patches\s*\(\s*const\s+TcClipPatchesParams\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"\bint64_t\s+tc_frames_from_u8_workspace\s*\(", header) and re.search(r"\bint64_t\s+tc_clip_patches_workspace\s*\(", header)
    doc = header[header.index("Pixel front end"):header.index("int tc_clip_patches(")]
    for cite in ("inference.py:64-69", "condition.py:322-330"):                   # what the entry points replace
        assert cite in doc, cite
    for word in ("TC_EINVAL", "TC_EWORKSPACE", "TC_ESHAPE", "HOST"):
        assert word in doc, word
    assert _lib.TC_FRAMES_U8_MAX == int(re.search(r"#define\s+TC_FRAMES_U8_MAX\s+(\d+)", header).group(1))


def test_ctypes_structs_match_the_compiled_header(tmp_path):
    """A probe compiled against the header prints sizeof and every offsetof; the ctypes mirrors must agree."""
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcFramesU8Params._fields_) == FRAMES_FIELDS
    assert tuple(f[0] for f in _lib.TcClipPatchesParams._fields_) == CLIP_FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %zu %zu", TC_ABI_VERSION, sizeof(TcFramesU8Params), sizeof(TcClipPatchesParams));']
    lines += [f'  printf(" %zu", offsetof(TcFramesU8Params, {f}));' for f in FRAMES_FIELDS]
    lines += [f'  printf(" %zu", offsetof(TcClipPatchesParams, {f}));' for f in CLIP_FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:3] == [14, ctypes.sizeof(_lib.TcFramesU8Params), ctypes.sizeof(_lib.TcClipPatchesParams)]
    assert got[3:3 + len(FRAMES_FIELDS)] == [getattr(_lib.TcFramesU8Params, f).offset for f in FRAMES_FIELDS]
    assert got[3 + len(FRAMES_FIELDS):] == [getattr(_lib.TcClipPatchesParams, f).offset for f in CLIP_FIELDS]


def test_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_frames_from_u8"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcFramesU8Params), ctypes.c_void_p])
    assert _lib.SYMBOLS["tc_clip_patches"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcClipPatchesParams), ctypes.c_void_p])
    assert _lib.load().tc_abi_version() == 14
    assert "pixel_front.hip" in build.SOURCES and "resize_tables.cpp" in build.SOURCES
    from tooncrafter_amd import clip
    from tooncrafter_amd.lvdm.openclip import VisionTransformer
    from tooncrafter_amd.ops import HipOps
    assert callable(HipOps.frames_from_u8) and callable(HipOps.clip_patches) and callable(VisionTransformer.tokens_from_patches)
    assert callable(clip.frames_from_uint8) and callable(clip.Conditions.from_uint8) and callable(clip.synthesize_u8)


# ---------------------------------------------------------------- the table builder and its statement

def test_resize_tables_equal_the_numpy_statement():
    """Bounds and every coefficient, over in, out in 1 .. 64, the full-HD frame widths both ways and the usual frame sides down
    to the model's; the columns of a row past its tap count are zero.  The statement divides by the filter scale where the
    library, like Pillow, multiplies by its reciprocal."""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    pairs = [(i, o) for i in range(1, 65) for o in range(1, 65)] + [(1920, 569), (569, 1920)]
    pairs += [(i, o) for i in (240, 360, 480, 720, 1080, 1440, 2160) for o in (320, 512, 576)]
    for n_in, n_out in pairs:
        bounds, coefs = c_tables(lib, n_in, n_out)
        want_b, want_c = pil_tables(n_in, n_out)
        assert coefs.shape == want_c.shape, (n_in, n_out)
        assert np.array_equal(bounds, want_b) and np.array_equal(coefs, want_c), (n_in, n_out)
    assert lib.tc_resize_tables(1920, 569, None, None, 0) == 9 and lib.tc_resize_tables(131, 16, None, None, 0) == 19


def test_the_statement_equals_pil():
    Image = pytest.importorskip("PIL.Image")
    for i, ((h, w), (oh, ow)) in enumerate(PIL_PAIRS):
        img = np.random.default_rng(6100 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(pil_resize(img, oh, ow), want), ((h, w), (oh, ow))


def test_resized_size_is_the_transform_rule():
    """tc_frames_from_u8_resized against the rule of the script's Resize(int) (dropin.py's shim): Python's int(s * long /
    short); and both sides change or neither, which is why tc_frames_from_u8 runs both passes or none."""
    from tooncrafter_amd.ops import HipOps
    hip = HipOps()
    for h, w in ((16, 24), (320, 512), (24, 16), (7, 7)):
        s = min(h, w)
        for sh in list(range(1, 70)) + [320, 720, 1080]:
            for sw in list(range(1, 70)) + [512, 1280, 1920]:
                if min(sh, sw) == s:
                    want = (sh, sw)
                elif sw < sh:
                    want = (int(s * sh / sw), s)
                else:
                    want = (s, int(s * sw / sh))
                got = hip.resized_size(sh, sw, h, w)
                assert got == want, (sh, sw, h, w)
                assert (got[0] != sh) == (got[1] != sw)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_resize_tables_refuses_bad_arguments():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    i32p = ctypes.POINTER(ctypes.c_int32)
    buf = np.full(64, -7, np.int32)
    ptr = buf.ctypes.data_as(i32p)
    assert lib.tc_resize_tables(0, 4, None, None, 0) == -1 and lib.tc_resize_tables(4, -1, None, None, 0) == -1
    assert lib.tc_resize_tables(8, 4, ptr, None, 64) == -1 and lib.tc_resize_tables(8, 4, None, ptr, 64) == -1
    assert lib.tc_resize_tables(8, 4, ptr, ptr, 4 * 5 - 1) == -4                 # kmax = 5: 20 coefficients
    assert (buf == -7).all()


def test_frames_from_u8_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    src = (ctypes.c_uint8 * (2 * 37 * 164))()
    out = (ctypes.c_float * (2 * 3 * 4 * 16 * 24))()
    tab = (ctypes.c_int32 * 256)()
    slots = (ctypes.c_int32 * 2)(0, 7)

    def rc(**kw):
        p = _lib.TcFramesU8Params(src=ctypes.addressof(src), image_stride=37 * 164, pitch=164, n=2, sh=37, sw=53, slots=slots,
                                  out=ctypes.addressof(out), b=2, t=4, h=16, w=24, h_kmax=7, v_kmax=7)
        p.h_bounds = p.h_coefs = p.v_bounds = p.v_coefs = ctypes.addressof(tab)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_frames_from_u8(ctypes.byref(p), None)
    assert lib.tc_frames_from_u8(None, None) == -1
    assert rc(src=None) == -1 and rc(out=None) == -1 and rc(slots=None) == -1
    assert rc(n=0) == -1 and rc(n=-2) == -1 and rc(n=_lib.TC_FRAMES_U8_MAX + 1) == -1
    assert rc(sh=0) == -1 and rc(sw=0) == -1 and rc(h=0) == -1 and rc(w=-3) == -1 and rc(b=0) == -1 and rc(t=0) == -1
    assert rc(pitch=3 * 53 - 1) == -1                                             # a row does not hold its pixels
    assert rc(image_stride=37 * 164 - 1) == -1                                    # images overlap
    assert rc(slots=(ctypes.c_int32 * 2)(0, 8)) == -1 and rc(slots=(ctypes.c_int32 * 2)(-1, 3)) == -1      # outside (b, t)
    assert rc(h_coefs=None) == -1 and rc(v_bounds=None) == -1 and rc(v_kmax=0) == -1      # resized, but a table is missing
    # 37 x 53 -> 16 x 22: the intermediate image is 2 * 37 * 22 * 3 bytes
    p = _lib.TcFramesU8Params(n=2, sh=37, sw=53, h=16, w=24)
    assert lib.tc_frames_from_u8_workspace(ctypes.byref(p)) == 2 * 37 * 22 * 3
    p.sh, p.sw = 16, 40                                                           # nothing to resize: no workspace
    assert lib.tc_frames_from_u8_workspace(ctypes.byref(p)) == 0
    assert rc(workspace=None, workspace_bytes=1 << 20) == -4
    assert rc(workspace=ctypes.addressof(tab), workspace_bytes=2 * 37 * 22 * 3 - 1) == -4
    assert not any(out) and not any(tab)


def test_clip_patches_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    x = (ctypes.c_float * (3 * 40 * 64))()
    out = (ctypes.c_uint16 * (4 * 592))()

    def rc(**kw):
        p = _lib.TcClipPatchesParams(x=ctypes.addressof(x), out=ctypes.addressof(out), b=1, h=40, w=64, size=28, patch=14, ld=592,
                                     antialias=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_clip_patches(ctypes.byref(p), None), lib.tc_clip_patches_workspace(ctypes.byref(p))
    assert lib.tc_clip_patches(None, None) == -1 and lib.tc_clip_patches_workspace(None) == 0
    assert rc(x=None)[0] == -1 and rc(out=None)[0] == -1
    assert rc(b=0)[0] == -1 and rc(h=0)[0] == -1 and rc(w=-1)[0] == -1 and rc(size=0)[0] == -1 and rc(patch=0)[0] == -1
    assert rc(ld=3 * 196 - 1)[0] == -1                                            # a row does not hold a patch
    assert rc(size=30)[0] == -3                                                   # S % patch != 0
    # reflect border: an axis the blur leaves alone still gets kornia's 3-tap kernel (sigma 0.001), one pixel each side
    assert rc(h=64, w=1)[0] == -3 and rc(h=1, w=64)[0] == -3
    assert rc(h=28 * 66, w=64)[0] == -3                                           # 131 taps: more than TC_CLIP_BLUR_TAPS
    # the blur needs two double copies of x; an upscale needs none (and is not refused for its workspace: it would launch)
    assert rc() == (-4, 2 * 3 * 40 * 64 * 8) and rc(workspace=ctypes.addressof(x), workspace_bytes=2 * 3 * 40 * 64 * 8 - 1)[0] == -4
    p = _lib.TcClipPatchesParams(x=ctypes.addressof(x), out=ctypes.addressof(out), b=1, h=20, w=20, size=28, patch=14, ld=592, antialias=1)
    assert lib.tc_clip_patches_workspace(ctypes.byref(p)) == 0
    p.h, p.w, p.antialias = 40, 64, 0
    assert lib.tc_clip_patches_workspace(ctypes.byref(p)) == 0
    assert not any(out)


# ---------------------------------------------------------------- the operator layer and the Python interface

def test_meta_kernels_infer_shape_and_dtype():
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    assert str(t.frames_from_u8.default._schema).startswith("tooncrafter::frames_from_u8(Tensor images, int[] slots, int b, int t, int h, int w,")
    assert str(t.clip_patches.default._schema).startswith("tooncrafter::clip_patches(Tensor x, int size, int patch, int ld, float[] mean,")
    def tabs(n_out):                                      # the tables of one resized axis: a row per output index
        return torch.empty(n_out, 2, dtype=torch.int32, device="meta"), torch.empty(n_out, 4, dtype=torch.int32, device="meta")
    from tooncrafter_amd import _lib
    rh, rw = ctypes.c_int32(), ctypes.c_int32()               # (37, 53) images are resized to (rh, rw) on the way to (16, 24)
    assert _lib.load().tc_frames_from_u8_resized(37, 53, 16, 24, ctypes.byref(rh), ctypes.byref(rw)) == 0
    assert (rh.value, rw.value) != (37, 53)
    imgs = torch.empty(2, 37, 53, 3, dtype=torch.uint8, device="meta")
    same = torch.empty(2, 16, 24, 3, dtype=torch.uint8, device="meta")          # keeps its size: no tables
    for src, tables in ((imgs, tabs(rw.value) + tabs(rh.value)), (same, (None,) * 4), (same, tabs(4) * 2)):
        y = t.frames_from_u8(src, [0, 3], 1, 4, 16, 24, *tables)
        assert y.shape == (1, 3, 4, 16, 24) and y.dtype == torch.float32 and y.device.type == "meta"
    for tables in ((None,) * 4, tabs(4) * 2):                 # a resize without its tables: refused as on the CUDA key
        with pytest.raises(RuntimeError, match="tables of"):
            t.frames_from_u8(imgs, [0, 3], 1, 4, 16, 24, *tables)
    for (b, h, w, size, patch, ld) in ((2, 40, 64, 28, 14, 592), (1, 320, 512, 224, 14, 592)):
        y = t.clip_patches(torch.empty(b, 3, h, w, device="meta"), size, patch, ld, [0.5, 0.5, 0.5], [0.25, 0.25, 0.25], True)
        assert y.shape == (b * (size // patch) ** 2, ld) and y.dtype == torch.bfloat16 and y.device.type == "meta"
    with pytest.raises((RuntimeError, NotImplementedError)):                      # no CPU kernel is registered: no fallback
        t.frames_from_u8(torch.zeros(1, 5, 7, 3, dtype=torch.uint8), [0], 1, 1, 16, 24, None, None, None, None)
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.clip_patches(torch.zeros(1, 3, 20, 20), 28, 14, 592, [0.5] * 3, [0.25] * 3, True)


def test_python_interface_rejects_wrong_dtypes_and_layouts():
    from tooncrafter_amd import clip
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    u8 = torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    for bad in (u8.float(), u8.to(torch.int8), u8[0], u8.permute(0, 3, 1, 2), u8[..., :2], "frame"):
        with pytest.raises(ValueError):
            clip.frames_from_uint8(bad, (16, 24), [(0, 0), (0, 3)], 4)
        with pytest.raises(ValueError):
            clip.Conditions.from_uint8(None, bad, u8, size=(16, 24), t=4)
        with pytest.raises(ValueError):
            clip.Conditions.from_uint8(None, u8, bad, size=(16, 24), t=4)
    with pytest.raises(ValueError):
        clip.Conditions.from_uint8(None, u8, u8[:1], size=(16, 24), t=4)          # one last frame for two first frames
    for slots in ([(0, 0)], [(0, 0), (0, 4)], [(0, 0), (-1, 1)], [(0, 0), (0, 1), (0, 2)]):
        with pytest.raises(ValueError):
            clip.frames_from_uint8(u8, (16, 24), slots, 4)
    with pytest.raises(ValueError):
        clip.frames_from_uint8(u8, (16, 0), [(0, 0), (0, 3)], 4)
    with pytest.raises(ValueError):                                               # pixels not packed: a channel-sliced view
        clip.frames_from_uint8(torch.zeros(2, 5, 7, 4, dtype=torch.uint8)[..., :3], (16, 24), [(0, 0), (0, 3)], 4)
    with pytest.raises(TooncrafterHipError):                                      # a well-formed CPU tensor: no fallback
        clip.frames_from_uint8(u8, (16, 24), [(0, 0), (0, 3)], 4)
    hip = HipOps()
    x = torch.zeros(1, 3, 20, 20)
    for bad in (dict(x=x.double()), dict(x=x[0]), dict(x=x[:, :2]), dict(size=30), dict(ld=587), dict(mean=(0.5, 0.5))):
        kw = dict(x=x, size=28, patch=14, ld=592, mean=(0.5,) * 3, std=(0.25,) * 3)
        kw.update(bad)
        with pytest.raises((ValueError, TooncrafterHipError)):
            hip.clip_patches(kw.pop("x"), **kw)


def test_tokens_from_patches_is_tokens_from_the_gemm_on():
    """On the emulated operator contract: the rows `tokens` unfolds, handed to `tokens_from_patches`, give its result."""
    from emu_ops import EmuOps
    from test_host_logic_cpu import _tiny_towers
    from tooncrafter_amd import ops
    prev = ops.set_backend(EmuOps(round_bf16=True))
    try:
        vis, _ = _tiny_towers()
        img = torch.randn(2, 3, 42, 42, generator=torch.Generator().manual_seed(3))
        pat = img.reshape(2, 3, 3, 14, 3, 14).permute(0, 2, 4, 1, 3, 5).reshape(18, 588)
        with torch.no_grad():
            a = torch.zeros((18, vis.pk["wc"].shape[1]), dtype=torch.bfloat16)
            a[:, :588] = pat.to(torch.bfloat16)
            assert torch.equal(vis.tokens_from_patches(a), vis.tokens(img))
            for bad in (a.float(), a[:17], a[:, :584], a[0]):
                with pytest.raises(ValueError):
                    vis.tokens_from_patches(bad)
    finally:
        ops.set_backend(prev)


# ---------------------------------------------------------------- the fixture

def test_pixel_front_fixture_is_what_the_generator_writes(tmp_path):
    pytest.importorskip("PIL.Image")
    out = tmp_path / "pixel_front.npz"
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_pixel_front_golden.py"), "--out", str(out)], check=True,
                   capture_output=True, env=env, timeout=300)
    new, old = dict(np.load(out)), load_golden("pixel_front.npz")
    assert sorted(new) == sorted(old)
    for k in sorted(old):
        assert new[k].shape == old[k].shape and new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN, "pixel_front.npz")) < 200 * 1024
