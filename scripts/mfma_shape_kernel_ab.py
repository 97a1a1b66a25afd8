#!/usr/bin/env python3
"""Per-kernel A/B of the MFMA shape of the tiled GEMM K loops (TC_GEMM_MFMA = 32 | 16: csrc/gemm.hip, csrc/gemm8.hip): wall
time AND engine clock per arm, one shape at a time, sustained, random data -- the clock is the hypothesis (the chip holds a
higher clock on v_mfma_f32_16x16x32_bf16 than on v_mfma_f32_32x32x16_bf16 at equal cycles).

The probes are those of scripts/clock_insitu.py (scripts/probes/clock_probe.hip, built into scripts/bin/libclock_probe.so):
engine clock = d(clock64) / d(wall_clock64) x 100 MHz between two in-stream probes, duration from the same 100 MHz counter.
The arms alternate, ROUNDS times each, so the spread of one arm's rounds stands beside the difference of the arms.  The
level-1 halo 3x3 convolution (csrc/conv_halo.hip: not behind the switch) is the control and must not move.  How far
the arms' outputs are apart is printed too (the two shapes round alike on most data: bit-identical outputs are no sign
that the switch was not read -- the times are).
usage: python scripts/mfma_shape_kernel_ab.py [--var TC_GEMM_MFMA] [--rounds 3] > profiles/mfma_shape_kernel_ab.txt"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tooncrafter_amd import ops  # noqa: E402
from tooncrafter_amd._lib import ACT_GEGLU  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--var", default="TC_GEMM_MFMA")
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
lib = ctypes.CDLL(os.path.join(ROOT, "scripts", "bin", "libclock_probe.so"))
lib.clk_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.clk_probe.restype = ctypes.c_int
slots = torch.zeros(4096, 2, dtype=torch.int64, device=dev)
_next = [0]
BF = torch.bfloat16


def probe():
    i = _next[0]
    _next[0] += 1
    rc = lib.clk_probe(slots[i % len(slots)].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return i % len(slots)


NPROBE = 12


def sustained(fn, warm, n):
    """-> (engine MHz, microseconds per launch).  The shader-clock counter is not one counter: a probe reads the counter of
    the place its single wave lands on, and two probes that landed on different ones are apart by an arbitrary offset (the
    100 MHz counter is chip-wide).  So NPROBE probes stand on either side of the stretch; of their pairs only those on the
    same counter give a physical clock (the others are off by orders of magnitude or negative), and their median is taken."""
    for _ in range(warm):
        fn()
    a = [probe() for _ in range(NPROBE)]
    for _ in range(n):
        fn()
    b = [probe() for _ in range(NPROBE)]
    torch.cuda.synchronize()
    s = slots.cpu()
    mhz = []
    for i in a:
        for j in b:
            dw = int(s[j, 1] - s[i, 1])
            r = int(s[j, 0] - s[i, 0]) / dw * 100.0
            if 500.0 < r < 4000.0:
                mhz.append(r)
    mhz.sort()
    return (mhz[len(mhz) // 2] if mhz else float("nan")), int(s[b[0], 1] - s[a[-1], 1]) / 100.0 / n


def ab(tag, fn, flops):
    per = max(int(0.4e-3 * 2.5e15 * 0.3 / flops), 4)
    outs = {}
    for arm in ("32", "16"):
        os.environ[args.var] = arm
        outs[arm] = fn().clone()
    torch.cuda.synchronize()
    same = torch.equal(outs["32"], outs["16"])
    d = float((outs["32"].float() - outs["16"].float()).abs().max())
    res = {"32": [], "16": []}
    for _ in range(args.rounds):
        for arm in ("32", "16"):
            os.environ[args.var] = arm
            res[arm].append(sustained(fn, warm=per * 100, n=per * 100))
    os.environ.pop(args.var, None)
    med = {arm: sorted(r[1] for r in res[arm])[len(res[arm]) // 2] for arm in res}
    spread = (max(r[1] for r in res["32"]) - min(r[1] for r in res["32"])) / med["32"]
    print(f"{tag}")
    for arm in ("32", "16"):
        print(f"    arm {arm}: " + " | ".join(f"{us:8.1f} us @ {mhz:5.0f} MHz" for mhz, us in res[arm])
              + f"   ({flops / med[arm] / 1e6:6.0f} TFLOP/s at the median)")
    print(f"    16 vs 32: time x{med['16'] / med['32']:.3f} ({100.0 * (med['32'] / med['16'] - 1.0):+.1f} %), clock x"
          f"{sum(r[0] for r in res['16']) / sum(r[0] for r in res['32']):.3f}; spread of arm 32 {100.0 * spread:.1f} %; "
          f"outputs max-abs apart {d:.3e}" + (" (bit-identical)" if same else ""), flush=True)


hip = ops.backend()
print(f"# {args.var} = 32 | 16, sustained, {args.rounds} alternating rounds per arm; device {torch.cuda.get_device_name(0)}; "
      f"{hip.lib.tc_build_info().decode()}")


def lin(m, n, k, tag, res=False, geglu=False):
    a = torch.randn(m, k, device=dev).to(BF)
    w = (torch.randn(n, k, device=dev) * k ** -0.5).to(BF)
    kw = {}
    if res:
        kw["residual"] = torch.randn(m, n, device=dev).to(BF)
    if geglu:
        kw["act"] = ACT_GEGLU
    bias = torch.randn(n, device=dev)
    ab(f"linear {tag} {m}x{n}x{k}" + (" + residual" if res else "") + (" GEGLU" if geglu else ""), lambda: hip.gemm(a, w, bias, **kw), 2.0 * m * n * k)


def t3(frames, hw, cin, n, tag):
    x = torch.randn(frames * hw, cin, device=dev).to(BF)
    w = (torch.randn(n, 3 * cin, device=dev) * (3 * cin) ** -0.5).to(BF)
    b = torch.randn(n, device=dev)
    geom = dict(kind="t3", frames=frames, t_len=16, cin=cin, h_out=1, w_out=hw)
    ab(f"conv t3 {tag} {frames * hw}x{n}x{3 * cin}", lambda: hip.gemm(x, w, b, conv=geom), 2.0 * frames * hw * n * 3 * cin)


def c3(frames, h, w_, cin, n, tag):
    x = torch.randn(frames * h * w_, cin, device=dev).to(BF)
    w = (torch.randn(n, 9 * cin, device=dev) * (9 * cin) ** -0.5).to(BF)
    b = torch.randn(n, device=dev)
    geom = dict(kind="3x3", frames=frames, cin=cin, h_in=h, w_in=w_, h_out=h, w_out=w_, stride=1, upsample=False)
    ab(f"conv 3x3 {tag} {cin}->{n}", lambda: hip.gemm(x, w, b, conv=geom), 2.0 * frames * h * w_ * n * 9 * cin)


def qkv(b, hw, c, tag):
    from tooncrafter_amd.lvdm.common import pack_linear
    x = torch.randn(b * 16 * hw, c, device=dev).to(BF)
    w = pack_linear(torch.randn(3 * c, c, device=dev) * c ** -0.5)
    ab(f"qkv + temporal attention {tag} B={b} hw={hw} C={c}", lambda: hip.temporal_qkv_attn(x, w, None, b=b, t=16, hw=hw, heads=c // 64),
       2.0 * b * 16 * hw * 3 * c * c)


with torch.no_grad():
    if args.var == "TC_QKV_MFMA":
        qkv(2, 640, 640, "L1")
        qkv(2, 160, 1280, "L2")
        qkv(2, 40, 1280, "L3")
        lin(20480, 1920, 640, "L1 qkv GEMM (control)")
        sys.exit(0)
    lin(20480, 1920, 640, "L1 qkv")
    lin(20480, 5120, 640, "L1 ff1", geglu=True)
    lin(5120, 1280, 1280, "L2 proj", res=True)
    lin(20480, 640, 640, "L1 proj", res=True)
    t3(32, 2560, 320, 320, "L0")
    t3(32, 40, 1280, 1280, "L3")
    c3(32, 20, 32, 640, 640, "L1 halo (control)")
