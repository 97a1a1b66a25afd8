"""CPU restatement of the 8-bit spatial self-attention (csrc/attention_q8.hip, ABI 14).

TEST INFRASTRUCTURE ONLY.  The reference has no 8-bit attention: what is restated here is the format and the tile
schedule the kernel's header states, so that the kernel can be pinned to it (the quantisers bit for bit, the attention to
fp32 summation-order tolerance) and the format choice can be measured on the CPU:

* K and Q rows: int8, one fp32 scale per (row, head): inv = 127 / amax, x_q = clamp(rint(x * inv), -127, 127),
  scale = amax / 127 (amax == 0: inv = 0, scale = 1);
* V^T: MXFP8 along the key axis, i.e. oracle.mx.quantize_mxfp8 of V^T with the keys zero-padded to whole 64-key tiles;
* the attention, tile by tile (64 keys): running max m per query, fp32 rescale of the accumulator, P quantised per query
  and 32-key block to e4m3 with the E8M0 exponent e = max(floor(blockmax(s') - m) - 8, -127) taken from the scores
  (s' = score * scale * log2 e), P_q = e4m3(min(exp2(s' - (m + e)), 448)) * 2^e, and the row sum l = the sum of the fp32 P
  (before the e4m3 rounding).

Every quantiser can be replaced by the identity (`qk=None, pv_mx=False`): the schedule is then exactly softmax attention.
"""
from __future__ import annotations

import math

import torch

from oracle import mx

KT = 64
REC = 9216
LOG2E = 1.4426950408889634


def quant_rows_i8(x: torch.Tensor):
    """x [rows, 64] (bf16 values) -> (int8 [rows, 64], fp32 scale [rows]), the kernel's formula in fp32."""
    x = x.to(torch.float32)
    amax = x.abs().amax(dim=1)
    pos = amax > 0
    one = torch.ones_like(amax)
    inv = torch.where(pos, torch.tensor(127.0, dtype=torch.float32) / torch.where(pos, amax, one), torch.zeros_like(amax))
    s = torch.where(pos, amax / torch.tensor(127.0, dtype=torch.float32), one)
    q = torch.round(x * inv[:, None]).clamp(-127, 127).to(torch.int8)
    return q, s


def quant_vt_mx(v: torch.Tensor):
    """v [lk, 64] -> (e4m3 bytes [64, lk_pad], E8M0 bytes [64, lk_pad / 32]) of V^T, keys zero-padded to 64."""
    lk = v.shape[0]
    pad = -(-lk // KT) * KT
    vt = torch.zeros(64, pad, dtype=torch.float32)
    vt[:, :lk] = v.to(torch.float32).t()
    return mx.quantize_mxfp8(vt)


def pack_records(k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """The workspace of one (batch, head) as tc_attn_q8_quant_kv writes it: uint8 [n_tiles, 9216] (layout: the kernel
    source's header; bytes past 8576 of a record are padding and come out zero here)."""
    lk = k.shape[0]
    nt = -(-lk // KT)
    kq, ks = quant_rows_i8(k)
    kqp = torch.zeros(nt * KT, 64, dtype=torch.int8)
    kqp[:lk] = kq
    ksp = torch.zeros(nt * KT, dtype=torch.float32)
    ksp[:lk] = ks
    vq, vs = quant_vt_mx(v)
    out = torch.zeros(nt, REC, dtype=torch.uint8)
    lane = torch.arange(64)
    l31, hh = lane % 32, lane // 32
    j = torch.arange(16)
    for t in range(nt):
        rec = out[t]
        kt = kqp[t * KT:(t + 1) * KT].view(torch.uint8)
        for kbk in range(2):
            for kk in range(2):
                f = kbk * 2 + kk
                rows = 32 * kbk + l31[:, None]
                cols = 32 * kk + 16 * hh[:, None] + j[None, :]
                rec[f * 1024:(f + 1) * 1024] = kt[rows, cols].reshape(-1)
        for d0 in range(2):
            for blk in range(2):
                f = d0 * 2 + blk
                keys = t * KT + 32 * blk + (j[None, :] & 3) + 8 * (j[None, :] >> 2) + 4 * hh[:, None]
                dims = 32 * d0 + l31[:, None]
                rec[4096 + f * 1024:4096 + (f + 1) * 1024] = vq[dims, keys].reshape(-1)
        rec[8192:8448] = ksp[t * KT:(t + 1) * KT].view(torch.uint8)
        rec[8448:8576] = vs[:, 2 * t:2 * t + 2].reshape(-1)
    return out


def _e4m3_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.float8_e4m3fn).to(x.dtype)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, *, qk="int8", pv_mx=True,
              dtype=torch.float32) -> torch.Tensor:
    """One (batch, head): q [lq, 64], k, v [lk, 64] -> o [lq, 64] in `dtype`, tile-faithful.
    qk: "int8" (the kernel), "mx" (MXFP8 e4m3 operands), "bf16" / None (the operands as given); pv_mx: MXFP8 P and V^T."""
    lq, lk = q.shape[0], k.shape[0]
    f32 = torch.float32
    if qk == "int8":
        qq, sq = quant_rows_i8(q)
        kq, sk = quant_rows_i8(k)
        acc = (qq.to(torch.float64) @ kq.to(torch.float64).t()).to(f32)          # exact integers (< 2^24)
        s = (acc * sk[None, :]).to(dtype)
        cq = ((torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)) * sq).to(dtype)[:, None]
    else:
        if qk == "mx":
            qd, kd = mx.fake_quant(q.to(f32)), mx.fake_quant(k.to(f32))
        else:
            qd, kd = q, k
        s = (qd.to(torch.float64) @ kd.to(torch.float64).t()).to(dtype)
        cq = torch.full((lq, 1), scale * LOG2E, dtype=torch.float64).to(dtype)
    if pv_mx:
        vq, vs = quant_vt_mx(v)
        vd = mx.dequantize_mxfp8(vq, vs).t().to(dtype)                         # [lk_pad, 64]
    else:
        vd = torch.zeros(-(-lk // KT) * KT, 64, dtype=dtype)
        vd[:lk] = v.to(dtype)
    nt = -(-lk // KT)
    m = torch.full((lq, 1), -1e30, dtype=dtype)
    l = torch.zeros((lq, 1), dtype=dtype)
    o = torch.zeros((lq, 64), dtype=dtype)
    for t in range(nt):
        st = torch.full((lq, KT), -math.inf, dtype=dtype)
        n = min(KT, lk - t * KT)
        st[:, :n] = s[:, t * KT:t * KT + n]
        bmx = st.view(lq, 2, 32).amax(dim=2)                                    # [lq, 2]
        m_new = torch.maximum(m, bmx.amax(dim=1, keepdim=True) * cq)
        alpha = torch.exp2(m - m_new)
        l, o, m = l * alpha, o * alpha, m_new
        e = torch.clamp(torch.floor(bmx * cq - m) - 8, min=-127)               # [lq, 2]
        mb = (m + e).repeat_interleave(32, dim=1)                               # [lq, 64]
        pv = torch.exp2((st.to(torch.float64) * cq.to(torch.float64) - mb.to(torch.float64)).to(dtype))
        scl = torch.exp2(e.to(torch.float64)).to(dtype)
        l = l + (pv.view(lq, 2, 32).sum(dim=2) * scl).sum(dim=1, keepdim=True)
        if pv_mx:
            pv = _e4m3_round(torch.clamp(pv, max=448.0))
        p = (pv.view(lq, 2, 32) * scl[:, :, None]).reshape(lq, KT)
        o = o + p @ vd[t * KT:(t + 1) * KT]
    return o / l


def attention_rows(q, k, v, *, batch, heads, lq, lk, scale, **kw) -> torch.Tensor:
    """Rows layout of ops.attention_q8: q [batch*lq, heads*64], k / v [batch*lk, heads*64] -> fp32 [batch*lq, heads*64]."""
    out = torch.empty(batch * lq, heads * 64, dtype=kw.get("dtype", torch.float32))
    for b in range(batch):
        for h in range(heads):
            cs = slice(h * 64, h * 64 + 64)
            out[b * lq:(b + 1) * lq, cs] = attention(q[b * lq:(b + 1) * lq, cs], k[b * lk:(b + 1) * lk, cs],
                                                     v[b * lk:(b + 1) * lk, cs], scale, **kw)
    return out


def softmax_attention(q, k, v, scale) -> torch.Tensor:
    """fp64 softmax(q k^T * scale) v of one (batch, head)."""
    s = (q.double() @ k.double().t()) * scale
    return torch.softmax(s, dim=1) @ v.double()
