#!/usr/bin/env python3
"""Workload for rocprofv3 --pmc passes (scripts/pmc_run.sh attn_q8 scripts/pmc_attn_q8.py attn_d64) over the level-0
spatial self-attention shape (b32 h5 2560^2): the bf16 kernel (tc_attn_d64) and the 8-bit route (ABI 14), twice each."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tooncrafter_amd.ops import HipOps  # noqa: E402

hip = HipOps()
b, h, L = 32, 5, 2560
qkv = torch.randn(b * L, 3 * h * 64, device="cuda").to(torch.bfloat16)
q, k, v = qkv[:, :320], qkv[:, 320:640], qkv[:, 640:]
for _ in range(2):
    hip.attention(q, k, v, batch=b, heads=h, lq=L, lk=L, scale=0.125)
    hip.attention_q8(q, k, v, batch=b, heads=h, lq=L, lk=L, scale=0.125)
torch.cuda.synchronize()
