"""Frame deltas and shot labels, everything that needs no GPU: the declaration, layout and export of the C ABI
(tc_frame_deltas), every refusal (before any launch, so host pointers do), the numpy statement of tests/frame_delta_ref.py on
its own (the exact consequences), `label_shots` on hand-made tables with ties exactly on each threshold, `ShotPlan.distinct`,
the wiring of `shots=` through the timeline on a recording backend, and the compile of csrc/frame_delta.hip without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import frame_delta_ref as ref
from conftest import ROOT
from test_colour_match_cpu import Spy

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
FIELDS = ("y", "c0", "c1", "image_stride_y", "image_stride_c", "pitch_y", "pitch_c", "format", "n", "h", "w", "lag", "tau", "hist",
          "delta", "workspace", "workspace_bytes")
RGB24, I420, NV12, P010 = 0, 1, 2, 3


# ---------------------------------------------------------------- declaration, layout, export

def test_header_declares_and_library_exports_and_binds_the_symbols():
    from tooncrafter_amd import _lib, build
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    for name in ("tc_frame_deltas_workspace", "tc_frame_deltas"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["tc_frame_deltas_workspace"] == (ctypes.c_int64, [ctypes.POINTER(_lib.TcFrameDeltaParams)])
    assert _lib.SYMBOLS["tc_frame_deltas"] == (ctypes.c_int, [ctypes.POINTER(_lib.TcFrameDeltaParams), ctypes.c_void_p])
    assert _lib.load().tc_abi_version() == 14 and _lib.TC_ABI_VERSION == 14       # additive: the version stays
    with open(HEADER) as f:
        header = f.read()
    assert "int64_t tc_frame_deltas_workspace(const TcFrameDeltaParams* p);" in header
    assert "int tc_frame_deltas(const TcFrameDeltaParams* p, void* stream);" in header
    assert "#define TC_DELTA_BINS 64" in header
    assert "frame_delta.hip" in build.SOURCES
    assert callable(HipOps.frame_deltas) and TorchLibOps.frame_deltas is HipOps.frame_deltas    # served by the inherited ctypes method


def test_ctypes_struct_matches_the_compiled_header(tmp_path):
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcFrameDeltaParams._fields_) == FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%d %d %d %zu", TC_ABI_VERSION, TC_DELTA_BINS, TC_PIXFMT_P010, sizeof(TcFrameDeltaParams));']
    lines += [f'  printf(" %zu", offsetof(TcFrameDeltaParams, {f}));' for f in FIELDS]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [14, 64, P010, ctypes.sizeof(_lib.TcFrameDeltaParams)]
    assert got[4:] == [getattr(_lib.TcFrameDeltaParams, f).offset for f in FIELDS]
    assert _lib.TC_DELTA_BINS == 64 == ref.BINS
    assert (_lib.TC_PIXFMTS["rgb24"], _lib.TC_YUV_FORMATS["i420"], _lib.TC_YUV_FORMATS["nv12"], _lib.TC_YUV_FORMATS["p010"]) == (0, 1, 2, 3)


# ---------------------------------------------------------------- refusals: before any device call, so host pointers do

def test_frame_deltas_refuses_bad_arguments_before_any_launch():
    from tooncrafter_amd import _lib
    lib = _lib.load()
    n, h, w = 3, 24, 40
    surf = (ctypes.c_uint8 * (n * h * w * 6 + 64))()
    hist = (ctypes.c_int32 * (n * 3 * 64 + 2))()
    delta = (ctypes.c_int64 * (n * 9 + 2))()
    ws = (ctypes.c_int64 * 4096)()
    S, H, D, W = (ctypes.addressof(v) for v in (surf, hist, delta, ws))
    layouts = {                                                                     # well-formed requests, one per format
        RGB24: dict(y=S, c0=None, c1=None, pitch_y=3 * w, image_stride_y=3 * w * h),
        I420: dict(y=S, c0=S + n * h * w, c1=S + 2 * n * h * w, pitch_y=w, image_stride_y=w * h, pitch_c=w // 2, image_stride_c=w * h // 4),
        NV12: dict(y=S, c0=S + n * h * w, c1=None, pitch_y=w, image_stride_y=w * h, pitch_c=w, image_stride_c=w * h // 2),
        P010: dict(y=S, c0=S + 2 * n * h * w, c1=None, pitch_y=2 * w, image_stride_y=2 * w * h, pitch_c=2 * w, image_stride_c=w * h),
    }

    def params(fmt, **kw):
        p = _lib.TcFrameDeltaParams(format=fmt, n=n, h=h, w=w, lag=1, tau=8, hist=H, delta=D, **layouts[fmt])
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rc(fmt, **kw):
        return lib.tc_frame_deltas(ctypes.byref(params(fmt, **kw)), None)

    def need(fmt, **kw):
        return lib.tc_frame_deltas_workspace(ctypes.byref(params(fmt, **kw)))
    assert lib.tc_frame_deltas(None, None) == -1 and lib.tc_frame_deltas_workspace(None) == 0
    for fmt in (RGB24, I420, NV12, P010):
        # well formed, no workspace: every one of these passes the argument checks and stops at the workspace
        for ok in ({}, dict(lag=2), dict(lag=3, delta=None), dict(lag=7, delta=None), dict(n=1, delta=None), dict(tau=0), dict(tau=255),
                   dict(h=23, w=39)):                                               # odd sizes: ch, cw round up and still fit the pitches
            assert rc(fmt, **ok) == -4, (fmt, ok)
            assert need(fmt, **ok) > 0
        assert rc(fmt, y=None) == -1 and rc(fmt, hist=None) == -1 and rc(fmt, delta=None) == -1
        for name in ("n", "h", "w"):
            assert rc(fmt, **{name: 0}) == -1 and rc(fmt, **{name: -2}) == -1, (fmt, name)
        assert rc(fmt, lag=0) == -1 and rc(fmt, lag=-1) == -1
        assert rc(fmt, tau=-1) == -1 and rc(fmt, tau=256) == -1
        assert rc(fmt, format=4) == -1 and rc(fmt, format=-1) == -1
        assert rc(fmt, pitch_y=layouts[fmt]["pitch_y"] - 1) == -1
        assert rc(fmt, image_stride_y=layouts[fmt]["image_stride_y"] - 1) == -1
        assert rc(fmt, hist=H + 2) == -2 and rc(fmt, delta=D + 4) == -2
        assert rc(fmt, delta=D + 4, lag=3) == -4                                   # no pair: delta is not looked at
        assert rc(fmt, workspace=None, workspace_bytes=1 << 30) == -4
        assert rc(fmt, workspace=W, workspace_bytes=need(fmt) - 1) == -4
        assert rc(fmt, workspace=W + 4, workspace_bytes=1 << 30) == -2
        for refused in (dict(y=None), dict(h=0), dict(tau=256), dict(hist=H + 2), dict(pitch_y=1)):
            assert need(fmt, **refused) == 0, (fmt, refused)
    # the chroma planes: presence as the format says, their pitches and strides
    assert rc(RGB24, c0=S) == -1 and rc(RGB24, c1=S) == -1
    assert rc(I420, c0=None) == -1 and rc(I420, c1=None) == -1
    assert rc(NV12, c0=None) == -1 and rc(NV12, c1=S) == -1 and rc(P010, c0=None) == -1 and rc(P010, c1=S) == -1
    for fmt in (I420, NV12, P010):
        assert rc(fmt, pitch_c=layouts[fmt]["pitch_c"] - 1) == -1 and rc(fmt, image_stride_c=layouts[fmt]["image_stride_c"] - 1) == -1
    assert rc(RGB24, pitch_c=0, image_stride_c=0) == -4                            # not read for RGB
    # P010: two-byte alignment of everything
    assert rc(P010, y=S + 1) == -2 and rc(P010, c0=layouts[P010]["c0"] + 1) == -2
    assert rc(P010, pitch_y=2 * w + 1, image_stride_y=(2 * w + 1) * h + 1) == -2 and rc(P010, image_stride_y=2 * w * h + 1) == -2
    assert rc(P010, pitch_c=2 * w + 1, image_stride_c=(2 * w + 1) * h) == -2 and rc(P010, image_stride_c=w * h + 1) == -2
    assert rc(NV12, y=S + 1) == -4 and rc(RGB24, y=S + 1) == -4                     # 8-bit planes need no alignment
    # sizes: more than 2^26 pixels; more than 2^31 - 1 blocks
    big = dict(pitch_y=3 * 8192, image_stride_y=3 * 8192 * 8193)
    assert rc(RGB24, h=8192, w=8192, pitch_y=3 * 8192, image_stride_y=3 * 8192 * 8192) == -4
    assert rc(RGB24, h=8193, w=8192, **big) == -3
    assert rc(RGB24, n=2 ** 31 - 1, lag=1) == -3 and rc(RGB24, n=2 ** 30, h=1, w=1, pitch_y=3, image_stride_y=3) == -3
    # the workspace: n * P * 3 * 66 int32, P the parts of an image: whole rows up to 32768 bytes, a row of more than 3 * 2^18 in segments
    one = 3 * 66 * 4
    assert need(RGB24) == n * 1 * one and need(I420) == n * 3 * one and need(NV12) == n * 2 * one == need(P010)
    assert need(RGB24, h=320, w=512, pitch_y=1536, image_stride_y=1536 * 320) == n * 16 * one        # 21 rows to a part
    assert need(NV12, n=1, delta=None, h=1080, w=1920, pitch_y=1920, image_stride_y=1920 * 1080, pitch_c=1920,
                image_stride_c=1920 * 540) == (64 + 32) * one                                          # 17 rows to a part
    assert need(RGB24, n=1, delta=None, h=2, w=2 ** 19, pitch_y=3 * 2 ** 19, image_stride_y=3 * 2 ** 20) == 2 * 2 * one
    assert not any(hist) and not any(delta) and not any(ws)


def test_the_binding_refuses_cpu_tensors_wrong_dtypes_and_arguments():
    from tooncrafter_amd import clip
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.torch_ops import TorchLibOps
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    planes = clip.Planes(torch.zeros(2, 8, 8, dtype=torch.uint8), (torch.zeros(2, 4, 4, 2, dtype=torch.uint8),), "nv12")
    for be in (HipOps(), TorchLibOps()):
        for frames in (x, planes):
            with pytest.raises(TooncrafterHipError):
                be.frame_deltas(frames)
            for bad in (dict(lag=0), dict(tau=-1), dict(tau=256)):
                with pytest.raises(ValueError):
                    be.frame_deltas(frames, **bad)
        for bad in (x.float(), x[..., :2], x[0], x.permute(0, 3, 1, 2)):
            with pytest.raises(ValueError):
                be.frame_deltas(bad)
    for bad in (x.float(), x[0], [x], None):
        with pytest.raises(ValueError):
            clip.frame_deltas(bad)
        with pytest.raises(ValueError):
            clip.find_shots(bad)
    with pytest.raises(ValueError):
        clip.find_shots(x, rule=0.5)


# ---------------------------------------------------------------- the statement on its own

@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_exact_consequences_of_the_statement(fmt):
    n, h, w = 3, 7, 9
    lay, total = ref.packed(fmt, n, h, w, pitch_quantum=16, gap=6)
    S = ref.samples(fmt, h, w)
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    comps = ref.components(buf, fmt, n, h, w, lay)
    assert [c.shape for c in comps] == [(n, s) for s in S]
    delta, hist = ref.deltas(comps, 1, 8)
    assert delta.shape == (2, 3, 3) and hist.shape == (3, 3, 64) and (hist.sum(axis=2) == np.array(S)).all()
    assert ref.deltas(comps, 3, 8)[0].shape == (0, 3, 3) and np.array_equal(ref.deltas(comps, 5, 8)[1], hist)
    # identical images: all zeros
    same = [np.repeat(c[:1], n, axis=0) for c in comps]
    assert not ref.deltas(same, 1, 0)[0].any() and not ref.deltas(same, 2, 0)[0].any()
    # 0 against 255
    flat = [np.stack([np.zeros(s, np.uint8), np.full(s, 255, np.uint8)]) for s in S]
    for tau in (0, 8, 254):
        d, hh = ref.deltas(flat, 1, tau)
        assert d.tolist() == [[[255 * s, s, 2 * s] for s in S]]
        assert (hh[0, :, 0] == np.array(S)).all() and (hh[1, :, 63] == np.array(S)).all() and hh.sum() == 2 * sum(S)
    assert ref.deltas(flat, 1, 255)[0][0, :, 1].tolist() == [0, 0, 0]               # nothing differs by MORE than 255
    # what the buffer holds between the rows is not read: change the padding after row 0 of the first plane, the numbers stay
    row = {"rgb24": 3 * w, "p010": 2 * w}.get(fmt, w)
    assert lay["pitch_y"] > row
    other = buf.copy()
    other[lay["y"] + row:lay["y"] + lay["pitch_y"]] ^= 0xFF
    d2, h2 = ref.deltas(ref.components(other, fmt, n, h, w, lay), 1, 8)
    assert np.array_equal(d2, delta) and np.array_equal(h2, hist)


def test_p010_reads_the_upper_byte_and_equals_nv12():
    n, h, w = 2, 5, 7
    rng = np.random.default_rng(6)
    lay8, total8 = ref.packed("nv12", n, h, w)
    v = rng.integers(0, 256, total8, dtype=np.uint8)
    lay16 = {k: 2 * x for k, x in lay8.items()}
    for low in (np.zeros(total8, np.uint16), rng.integers(0, 256, total8).astype(np.uint16)):
        words = (v.astype(np.uint16) << 8) | low
        buf = words.astype("<u2").view(np.uint8)
        a = ref.deltas(ref.components(buf, "p010", n, h, w, lay16), 1, 8)
        b = ref.deltas(ref.components(v, "nv12", n, h, w, lay8), 1, 8)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- labels

def test_label_shots_compares_exactly_on_every_threshold():
    from tooncrafter_amd import clip
    S = (1000, 250, 250)                                                           # 1500 samples in all
    rule = clip.ShotRule()
    assert (rule.tau, rule.hold_moved, rule.cut_hist, rule.cut_mad) == (8, 0.002, 0.35, 20.0)

    def label(sad, changed, l1, rule=rule):
        return clip.label_shots([[[sad[c], changed[c], l1[c]] for c in range(3)]], S, rule).labels[0]
    big = (30000, 0, 0)                                                            # mad = 20 exactly
    # moved = 3 / 1500 = 0.002 exactly: a hold; one more sample: not a hold
    assert label(big, (3, 0, 0), (700, 0, 0)) == "hold" and label(big, (1, 1, 1), (700, 0, 0)) == "hold"
    assert label(big, (4, 0, 0), (700, 0, 0)) == "cut" and label(big, (2, 1, 1), (100, 0, 0)) == "tween"
    # hist = 700 / 2000 = 175 / 500 = 0.35 exactly in component 0 or 1; one count less: a tween
    assert label(big, (9, 0, 0), (700, 0, 0)) == "cut" and label(big, (9, 0, 0), (0, 175, 0)) == "cut"
    assert label(big, (9, 0, 0), (698, 174, 174)) == "tween" and label(big, (9, 0, 0), (0, 0, 176)) == "cut"
    # mad = 30000 / 1500 = 20 exactly; one code value less in all: a tween
    assert label((10000, 10000, 10000), (9, 0, 0), (700, 0, 0)) == "cut" and label((29999, 0, 0), (9, 0, 0), (700, 0, 0)) == "tween"
    # a float that is not the decimal it was written as would miss these ties: 0.35 < 7/20 < float(0.35) is impossible in fractions
    third = clip.ShotRule(tau=0, hold_moved=0.1, cut_hist=0.7, cut_mad=0.3)
    assert label((450, 0, 0), (150, 0, 0), (1400, 0, 0), third) == "hold"          # 150 / 1500 = 0.1
    assert label((450, 0, 0), (151, 0, 0), (1400, 0, 0), third) == "cut"           # 1400 / 2000 = 0.7, 450 / 1500 = 0.3
    assert label((449, 0, 0), (151, 0, 0), (1400, 0, 0), third) == "tween" and label((450, 0, 0), (151, 0, 0), (1399, 0, 0), third) == "tween"
    # numbers past 2^53 stay exact
    huge = clip.label_shots([[[2 ** 62, 2 ** 60, 0]] * 3], (2 ** 60,) * 3, clip.ShotRule(hold_moved=1))
    assert huge.labels == ("hold",) and huge.moved == (1.0,) and huge.mad == (4.0,)
    plan = clip.label_shots([[[30000, 3, 700], [0, 0, 0], [0, 0, 0]], [[30000, 4, 700], [0, 0, 0], [0, 0, 0]],
                             [[29999, 4, 700], [0, 0, 0], [0, 0, 0]]], S)
    assert plan.labels == ("hold", "cut", "tween") and plan.moved == (0.002, 4 / 1500, 4 / 1500)
    assert plan.mad == (20.0, 20.0, 29999 / 1500) and plan.hist == (0.35, 0.35, 0.35)
    for bad in ((0, 1, 1), (1, 1), (1, 1, -1)):
        with pytest.raises(ValueError):
            clip.label_shots([], bad)
    with pytest.raises(ValueError):
        clip.label_shots([[[1, 2, 3]]], S)
    for bad in (dict(tau=-1), dict(tau=256), dict(tau=1.5), dict(tau=True), dict(hold_moved=-0.1), dict(cut_hist=float("nan")),
                dict(cut_mad=float("inf")), dict(cut_mad="20")):
        with pytest.raises(ValueError):
            clip.ShotRule(**bad)


def test_shot_plan_by_hand_and_distinct():
    from tooncrafter_amd import clip
    plan = clip.ShotPlan(["tween", "hold", "hold", "cut", "tween", "hold"])
    assert plan.labels == ("tween", "hold", "hold", "cut", "tween", "hold") and plan.moved is plan.mad is plan.hist is None
    assert plan.distinct() == [0, 1, 4, 5]
    assert clip.ShotPlan(()).distinct() == [0] and clip.ShotPlan(("hold",) * 3).distinct() == [0]
    assert clip.ShotPlan(("cut", "tween")).distinct() == [0, 1, 2]
    for bad in (("tween", "fade"), ("CUT",), (None,)):
        with pytest.raises(ValueError):
            clip.ShotPlan(bad)
    assert clip.component_samples(torch.zeros(2, 5, 7, 3, dtype=torch.uint8)) == (35, 35, 35)
    planes = clip.Planes(torch.zeros(2, 5, 7, dtype=torch.uint8), (torch.zeros(2, 3, 4, 2, dtype=torch.uint8),), "nv12")
    assert clip.component_samples(planes) == (35, 12, 12)


# ---------------------------------------------------------------- the timeline

class TimelineSpy(Spy):
    """the recording backend with a front end (image i becomes the constant of its first byte) and writers that count, per frame
    of the video, how often it is written, from the strides and the offset of `out` they are given"""

    def __init__(self, frame_bytes):
        super().__init__()
        self.frame_bytes, self.written, self.base = frame_bytes, {}, None

    def frames_from_u8(self, images, size, slots, *, b, t, out=None):
        self.calls.append(("frames_from_u8", tuple(images.shape), tuple(size), list(slots), b, t, int(images.flatten()[0])))
        x = torch.zeros(b, 3, t, *size)
        for i, s in enumerate(slots):
            x[s // t, :, s % t] = 100.0 + float(images[i].flatten()[0])
        return x

    def _mark(self, x, frames, out, strides):
        self.base = out.data_ptr() if self.base is None else min(self.base, out.data_ptr())
        f0, nf = frames
        for clip_i in range(x.shape[0]):
            for j in range(nf):
                at = out.data_ptr() + clip_i * strides[2] + j * strides[1]
                self.written.setdefault(at, []).append(float(x[clip_i, 0, f0 + j, 0, 0]))

    def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
        self._mark(x, frames, out, strides)
        return super().frames_to_u8(x, size, filter, fmt, frames, out, strides)

    def frames_to_yuv(self, x, size=None, filter="bicubic", fmt="nv12", colour=None, frames=None, out=None, strides=None):
        self._mark(x, frames, out, strides)
        return super().frames_to_yuv(x, size, filter, fmt, colour, frames, out, strides)

    def video(self, total):
        """per frame of the video: the values written there"""
        return [self.written.get(self.base + f * self.frame_bytes, []) for f in range(total)]


@pytest.fixture
def stub_pipeline(monkeypatch):
    """Conditions.from_uint8 / sample / decode_spliced replaced: a batch's decoded clip is the constant 1 + its first segment,
    clip j of it 1 + first segment + j, on (n, 3, 4, 6, 8) clips; every sample call is recorded with its seeds and prompts"""
    from tooncrafter_amd import clip, ops

    class Cond:
        refs = None

        def __init__(self, first, n, prompts):
            self.first, self.n, self.prompts = first, n, prompts
            self.ends_px = torch.full((n, 3, 2, 5, 7), 10.0 + first)
    sampled = []

    def from_uint8(model, first, last, *, size, t, prompts=None, **options):
        assert len(first) == len(last) and int(last[0, 0, 0, 0]) == int(first[0, 0, 0, 0]) + 1
        return Cond(int(first[0, 0, 0, 0]), len(first), prompts)

    def sample(model, cond, plan, latent_shape, pinned=None, variant=0):
        sampled.append((cond.first, cond.n, None if plan.seeds is None else list(plan.seeds), cond.prompts, list(latent_shape)))
        return cond

    def decode(model, cond, refs):
        return (1.0 + cond.first + torch.arange(cond.n, dtype=torch.float32)).view(-1, 1, 1, 1, 1).expand(cond.n, 3, 4, 6, 8).contiguous()
    monkeypatch.setattr(clip.Conditions, "from_uint8", staticmethod(from_uint8))
    monkeypatch.setattr(clip, "sample", sample)
    monkeypatch.setattr(clip, "decode_spliced", decode)
    spy = TimelineSpy(6 * 8 * 3)
    prev = ops.set_backend(spy)
    yield clip, spy, sampled
    ops.set_backend(prev)


def keyframes_u8(k):
    return torch.arange(k, dtype=torch.uint8).view(k, 1, 1, 1).expand(k, 8, 8, 3).contiguous()


def test_shots_none_records_the_same_calls_as_before(stub_pipeline):
    """the parent's call list for six keyframes in batches of two: segments (0, 1), (2, 3), (4), written by timeline_layout's rule"""
    clip, spy, sampled = stub_pipeline
    plan = clip.SamplingPlan(steps=2, seeds=[50, 51, 52, 53, 54])
    prompts = ["a", "b", "c", "d", "e"]
    clip.synthesize_timeline_u8(None, keyframes_u8(6), [2, 4, 4, 1, 1], size=(6, 8), plan=plan, prompts=prompts)
    assert sampled == [(0, 2, [50, 51], ["a", "b"], [2, 4, 4, 1, 1]), (2, 2, [52, 53], ["c", "d"], [2, 4, 4, 1, 1]),
                       (4, 1, [54], ["e"], [1, 4, 4, 1, 1])]
    assert spy.calls == [("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (0, 1), 1.0),
                         ("frames_to_u8", (2, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 1.0),
                         ("frames_to_u8", (2, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 3.0),
                         ("frames_to_u8", (1, 3, 4, 6, 8), None, "bicubic", "rgb24", (1, 3), 5.0)]
    assert spy.video(16) == [[1.0]] + [[1.0]] * 3 + [[2.0]] * 3 + [[3.0]] * 3 + [[4.0]] * 3 + [[5.0]] * 3
    with_none = list(spy.calls)
    spy.calls.clear()
    sampled.clear()
    clip.synthesize_timeline_u8(None, keyframes_u8(6), [2, 4, 4, 1, 1], size=(6, 8), plan=plan, prompts=prompts, shots=None)
    assert spy.calls == with_none and len(sampled) == 3


@pytest.mark.parametrize("planar", [False, True])
def test_a_shot_plan_samples_the_tween_runs_and_writes_every_frame_once(stub_pipeline, planar):
    from tooncrafter_amd.output import Colour
    clip, spy, sampled = stub_pipeline
    plan = clip.SamplingPlan(steps=2, seeds=[50, 51, 52, 53, 54])
    prompts = ["a", "b", "c", "d", "e"]
    shots = clip.ShotPlan(("tween", "cut", "tween", "tween", "hold"))
    extra = dict(out_fmt="nv12", out_colour=Colour("bt709")) if planar else {}
    spy.frame_bytes = 6 * 8 * 3 // 2 if planar else 6 * 8 * 3
    video = clip.synthesize_timeline_u8(None, keyframes_u8(6), [2, 4, 4, 1, 1], size=(6, 8), plan=plan, prompts=prompts, shots=shots,
                                        **extra)
    assert video.shape == ((16, 6 * 8 * 3 // 2) if planar else (16, 6, 8, 3))
    # the runs [0] and [2, 3], seeds and prompts by the ORIGINAL segment number; nothing else is sampled
    assert sampled == [(0, 1, [50], ["a"], [1, 4, 4, 1, 1]), (2, 2, [52, 53], ["c", "d"], [2, 4, 4, 1, 1])]
    # every frame of the video exactly once: sampled clips are 1 + segment, keyframe i comes through the front end as 100 + i
    assert spy.video(16) == [[1.0]] + [[1.0]] * 3 + [[101.0], [101.0], [102.0]] + [[3.0]] * 3 + [[4.0]] * 3 + [[104.0], [104.0], [105.0]]
    front = [c for c in spy.calls if c[0] == "frames_from_u8"]
    assert front == [("frames_from_u8", (2, 8, 8, 3), (6, 8), [0, 1], 1, 2, 1), ("frames_from_u8", (2, 8, 8, 3), (6, 8), [0, 1], 1, 2, 4)]
    assert not [c for c in spy.calls if c[0].startswith("colour")]
    # a batch of three does not join the runs across the cut either; a skipped segment 0 writes the video's frame 0
    for held in (spy.calls, sampled, spy.written):
        held.clear()
    spy.base = None
    clip.synthesize_timeline_u8(None, keyframes_u8(6), [3, 4, 4, 1, 1], size=(6, 8), plan=plan, prompts=prompts,
                                shots=clip.ShotPlan(("hold", "tween", "tween", "tween", "tween")), **extra)
    assert sampled == [(1, 3, [51, 52, 53], ["b", "c", "d"], [3, 4, 4, 1, 1]), (4, 1, [54], ["e"], [1, 4, 4, 1, 1])]
    assert spy.video(16) == [[100.0]] + [[100.0], [100.0], [101.0]] + [[2.0]] * 3 + [[3.0]] * 3 + [[4.0]] * 3 + [[5.0]] * 3


def test_a_match_is_applied_to_sampled_segments_only(stub_pipeline):
    from tooncrafter_amd.output import ColourMatch
    clip, spy, sampled = stub_pipeline
    clip.synthesize_timeline_u8(None, keyframes_u8(4), [2, 4, 4, 1, 1], size=(6, 8), plan=clip.SamplingPlan(steps=2),
                                shots=clip.ShotPlan(("cut", "tween", "hold")), match=ColourMatch("mkl", 0.5))
    assert [c[0] for c in spy.calls] == ["frames_from_u8", "frames_to_u8", "frames_to_u8", "frames_from_u8", "frames_to_u8",
                                         "colour_stats", "colour_stats", "colour_match", "frames_to_u8"]
    assert sampled == [(1, 1, None, None, [1, 4, 4, 1, 1])]
    assert spy.video(10) == [[100.0]] + [[100.0], [100.0], [101.0]] + [[1002.0]] * 3 + [[102.0], [102.0], [103.0]]


def test_bad_shots_raise_before_anything_is_launched(stub_pipeline):
    clip, spy, sampled = stub_pipeline
    plan = clip.SamplingPlan(steps=2)
    for bad in (clip.ShotPlan(("tween", "cut")), clip.ShotPlan(("tween",) * 4), "cut", ("tween", "cut", "tween"), 0.5):
        with pytest.raises(ValueError):
            clip.synthesize_timeline_u8(None, keyframes_u8(4), [2, 4, 4, 1, 1], size=(6, 8), plan=plan, shots=bad)
    forged = clip.ShotPlan(("tween", "cut", "tween"))
    object.__setattr__(forged, "labels", ("tween", "fade", "tween"))               # an unknown label that got past the constructor
    with pytest.raises(ValueError):
        clip.synthesize_timeline_u8(None, keyframes_u8(4), [2, 4, 4, 1, 1], size=(6, 8), plan=plan, shots=forged)
    assert not spy.calls and not sampled


def test_a_shot_rule_runs_find_shots_first(stub_pipeline, monkeypatch):
    clip, spy, sampled = stub_pipeline
    seen = []

    def frame_deltas(frames, lag=1, tau=8):
        seen.append((tuple(frames.shape), lag, tau))
        table = torch.zeros(3, 3, 3, dtype=torch.int64)
        table[1, :, 0], table[1, :, 1], table[1, :, 2] = 64 * 200, 64, 128          # segment 1: everything moved, histograms apart
        table[2, 0, 0], table[2, 0, 1] = 640, 32                                    # segment 2: half of one component moved a little
        return table, torch.zeros(4, 3, 64, dtype=torch.int32)
    spy.frame_deltas = frame_deltas
    found = clip.find_shots(keyframes_u8(4), clip.ShotRule(tau=3))
    assert found.labels == ("hold", "cut", "tween") and seen == [((4, 8, 8, 3), 1, 3)]
    assert found.moved == (0.0, 1.0, 32 / 192) and found.mad == (0.0, 200.0, 640 / 192) and found.hist == (0.0, 1.0, 0.0)
    clip.synthesize_timeline_u8(None, keyframes_u8(4), [2, 4, 4, 1, 1], size=(6, 8), plan=clip.SamplingPlan(steps=2), shots=clip.ShotRule(tau=5))
    assert seen[-1] == ((4, 8, 8, 3), 1, 5) and sampled == [(2, 1, None, None, [1, 4, 4, 1, 1])]


# ---------------------------------------------------------------- compilation

def test_frame_delta_hip_compiles_for_gfx950_without_scratch(tmp_path):
    from tooncrafter_amd import build
    src = os.path.join(build.CSRC, "frame_delta.hip")
    r = subprocess.run([build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fd.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {k for k in ("frame_delta_kernel", "frame_delta_finish_kernel") if any(k in n for n in names)}
    assert len(kernels) == 2 and len(names) == len(scratch) == 3, names             # the parts: two load forms; the finish
    assert scratch == [0] * 3, list(zip(names, scratch))
