#!/usr/bin/env python3
"""Time the bf16 spatial self-attention (tc_attn_d64) against the 8-bit route (tc_attn_q8_quant_kv + tc_attn_d64_q8, ABI 14)
at the four spatial self-attention shapes of the guided forward, interleaved in one process, q / k / v as column slices
of one [rows, 3C] qkv tensor as in the forward.  Also times the two 8-bit launches alone.

    python scripts/attn_q8_bench.py
"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tooncrafter_amd import _lib  # noqa: E402
from tooncrafter_amd.ops import HipOps  # noqa: E402


def timeit(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def main():
    hip = HipOps()
    g = torch.Generator().manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}  {hip.lib.tc_build_info().decode()}")
    for b, h, L in ((32, 5, 2560), (16, 5, 2560), (32, 10, 640), (32, 20, 160)):
        hd = h * 64
        qkv = (torch.randn(b * L, 3 * hd, generator=g) * 1.5).to(torch.bfloat16).cuda()
        q, k, v = qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]
        kw = dict(batch=b, heads=h, lq=L, lk=L, scale=0.125)
        out = torch.empty(b * L, hd, dtype=torch.bfloat16, device="cuda")
        p = hip._q8_params(q, k, v, out, b, h, L, L, 0.125)
        ws = torch.empty(hip.lib.tc_attn_q8_workspace(C.byref(p)), dtype=torch.uint8, device="cuda")
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        quant = lambda: _lib.check(hip.lib.tc_attn_q8_quant_kv(C.byref(p), 0), "quant")
        attn = lambda: _lib.check(hip.lib.tc_attn_d64_q8(C.byref(p), 0), "attn")
        rounds = [(timeit(lambda: hip.attention(q, k, v, **kw)), timeit(lambda: hip.attention_q8(q, k, v, **kw)))
                  for _ in range(4)][1:]
        t16 = sorted(r[0] for r in rounds)[1]
        t8 = sorted(r[1] for r in rounds)[1]
        tq, ta = timeit(quant), timeit(attn)
        fl = 4.0 * b * h * L * L * 64
        d = (hip.attention(q, k, v, **kw).float() - hip.attention_q8(q, k, v, **kw).float())
        rel = float(d.norm() / hip.attention(q, k, v, **kw).float().norm())
        print(f"b{b:3d} h{h:3d} {L:5d}^2: tc_attn_d64 {t16:7.1f} us ({fl / t16 * 1e-6:5.0f} TF/s) | 8-bit {t8:7.1f} us "
              f"(quant_kv {tq:6.1f} + attn {ta:7.1f}; {fl / ta * 1e-6:5.0f} TF/s in the attention)  x{t16 / t8:.3f}  "
              f"rel-L2 8-bit vs bf16 {rel:.2e}")


if __name__ == "__main__":
    main()
