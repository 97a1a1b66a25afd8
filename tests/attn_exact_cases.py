"""The table behind tests/test_attn_exact_cpu.py (no GPU) and tests/test_gpu_attn_exact.py (MI355X): attention problems on
which the correct output of a kernel is known TO THE BIT, for every attention kernel of the library.

Two input constructions make softmax(q k^T / 8) v predictable (head dim 64, scale 1/8):

  gather   keys are A kappa(j) with distinct +-1 code vectors kappa over the head's dims, query i is A kappa(pi(i)) for a chosen
           target map pi.  With A = 8 the target's score is 512 and every other score lower by A^2 (64 - kappa.kappa') / 8
           >= 192, so in fp32 the other weights are 0 (or denormal), P rounds to 1.0 in bf16 (and in e4m3 behind its block
           exponent) and the row sum is 1 to 2^-30: the stored output is EXACTLY v[pi(i)] plus what the operator adds (the
           accumulate base, the second key/value set's v2[pi2(i)], the relative table row Rv[idx]).  Every query row, key
           slot, head, batch -> K/V batch mapping and mask boundary is then held to the bit.
           (Dual key/value sets: the codes of set 1 live on dims 0..31 and those of set 2 on dims 32..63, A = 16, so that one
           query row carries two independent targets; relative "gather by distance": all keys equal, Rk[c] = A kappa(c), and
           the query carries the code of its target's distance.)
  equal    all keys of a (batch, head) are ONE non-zero vector, so every visible key has the same score whatever the query:
           each key must be counted exactly once and no padded key at all.  V[k][j] = c_j + s_kj d_j with non-zero integers
           c, d and signs s in {+1, -1, 0} that sum to zero over the valid keys of every dim j (one zero-sum sign sequence,
           rotated by a seeded number of keys in each dim j, so that the V rows differ).  Where the kernel keeps the weights un-normalised (the
           flash kernels, attn_tile64.h tc_tile64_softmax / tc_tile64_store: P = exp2(..) in bf16, O / l once at the end) or in
           fp32 (attention.hip attn_temporal_kernel: "s[j] * inv"), the stored output is exactly c_j.  The MFMA temporal cores
           round the NORMALISED weight to bf16 (attn_frames16.h "pack2(e[0] * inv, ..)", attn_frames_long.h
           "pf[j] = (bf16_t)(st[kb][8 * s + j] * inv)"; attention_temporal_rel.hip: "Roundings: .. bf16 softmax weights and
           bucket sums, fp32 sums, bf16 output"): there the output is exactly rne_bf16(bf16(1 / n) * sum_k v_k) with n the
           number of visible keys -- every product and the sum are exact in fp32.

expected(case, inp) is a float64 softmax with exactly those rounding points; closed_form(case, inp) is the same answer
written down without any attention arithmetic (v[pi], c, the bf16(1/n) formula).  test_attn_exact_cpu.py holds the two equal
for every case, holds every case to the conditions below and shows, per seeded defect (DEFECTS), the cases whose expected
output it changes.  Neither function calls code under test, and nothing here depends on tests/emu_ops.py.

Conditions (validate(case, inp) -> list of violations):
  * gather mass: the float64 softmax gives the target 1 - w < 2^-30 for every query;
  * every expected output and every intermediate sum the operator forms (v + base, v1 + v2, v + Rv) is an integer of
    magnitude <= 256 (gather) -- bf16 holds it exactly; equal-weight outputs are bf16 values by construction of the formula;
  * attention_q8: |v| <= 14 (an amax of 15 maps to 480 under the MXFP8 block scale, beyond e4m3's 448);
  * no two V rows one query can see are equal, and the V rows (gather) / the c vectors (equal) of different heads and batches
    differ;
  * pi is not the identity, not monotone, not the same for two heads or two batches (wherever lk > 2 leaves room); its targets
    are as many distinct keys as lq allows and include the last valid key;
  * MFMA cores, equal weights: 1 / n for n = 1 .. 64 lies farther than 2^-20 (relative) from every bf16 rounding midpoint, so
    the 1-ulp v_rcp_f32 cannot change bf16(1 / n) (midpoint_margin()).
"""
from dataclasses import dataclass

import torch

BF16 = torch.bfloat16
F64 = torch.float64
SENTINEL = 7.0
SCALE = 0.125
D = 64

# the seeded defects of test_attn_exact_cpu.py -> the operators they concern
ALL_OPS = ("attention", "attention_q8", "temporal", "temporal_rel", "qkv_attn", "tb_fused")
DEFECTS = {
    "pad_key": ("attention", "attention_q8", "temporal", "temporal_rel"),       # one padded key counted (zero key and value)
    "drop_last": ("attention", "attention_q8", "temporal", "temporal_rel", "qkv_attn"),   # last valid key of a ragged tile dropped
    "swap_p": ALL_OPS,                          # keys +4..7 and +8..11 of a 16-key step swapped for P but not for V
    "bdiv_mod": ("attention",),                 # b % kv_bdiv in place of b // kv_bdiv
    "head_swap_v": ALL_OPS,                     # heads h and h + 1 exchanged for V only
    "skip_row127": ("attention", "attention_q8"),   # the last query row of a 128-row block not written
    "causal_ge": ("temporal_rel",),             # mask j >= i in place of j > i
    "rel_off1": ("temporal_rel",),              # relative index off by one
    "no_clamp": ("temporal_rel",),              # the clamp at L missing (the index wraps in the table)
}


@dataclass(frozen=True)
class Case:
    name: str
    op: str                     # attention | attention_q8 | temporal | temporal_rel | qkv_attn | tb_fused
    kind: str                   # gather | equal | gather_dist (temporal_rel: the code sits in Rk)
    target: str                 # the kernel the call runs
    family: str                 # flash (un-normalised bf16 P) | valu (fp32) | mfma (normalised bf16 P)
    batch: int = 1              # spatial: query batches; temporal: clips
    heads: int = 1
    lq: int = 0                 # spatial
    lk: int = 0
    kv_bdiv: int = 1
    lk2: int = 0                # second key/value set (0: none)
    kv2_bdiv: int = 1
    accumulate: bool = False
    packed: bool = False        # q, k, v are column slices of one [rows, 3C] buffer, out is a column slice as well
    t: int = 0                  # temporal
    hw: int = 0
    max_rel: int = 0
    causal: bool = False
    tables: bool = False        # relative tables given
    zero_tables: bool = False   # ... and all zero

    @property
    def spatial(self):
        return self.op in ("attention", "attention_q8")

    @property
    def tile(self):
        """keys per masked tile: what 'ragged' means for this kernel"""
        return 64 if self.spatial else 16 if (self.family == "valu" or self.t <= 16) else 32


# ---------------------------------------------------------------------------------------------------------------- helpers
def _seed(c, salt=0):
    return (sum((i + 1) * ord(ch) for i, ch in enumerate(c.name)) * 64 + salt) % (2 ** 31)


def _gen(c, salt=0):
    return torch.Generator().manual_seed(_seed(c, salt))


def _signs(g, *shape):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def rne_bf16(x):
    """float64 -> the bf16 value (as float64), through fp32 like every store of the library"""
    return x.float().to(BF16).double()


def midpoint_margin(n_max=64):
    """min over n = 1 .. n_max of the relative distance of 1 / n from the nearest bf16 rounding midpoint"""
    worst = 1.0
    for n in range(1, n_max + 1):
        x = 1.0 / n
        e = torch.floor(torch.log2(torch.tensor(x, dtype=F64))).item()
        ulp = 2.0 ** (e - 7)
        frac = (x / ulp) % 1.0                    # position inside the bf16 interval, midpoint at 0.5
        worst = min(worst, abs(frac - 0.5) * ulp / x)
    return worst


def make_pi(n_q, n_k, salt, causal=False, max_dist=None):
    """Target map [n_q] -> [0, n_k): a stride walk through the keys (stride coprime to n_k, near 0.38 n_k: neither the identity
    nor monotone), offset by `salt`; one query is redirected to the last key when the walk misses it; for 3 .. 6 keys one of
    the non-trivial permutations.  causal (pi(i) <= i, with pi(i) == i for some i > 0) and max_dist (|pi(i) - i| < max_dist):
    seeded draws inside the allowed span instead."""
    i = torch.arange(n_q)
    if causal or max_dist is not None:
        g = torch.Generator().manual_seed(7919 * n_q + 31 * salt + (17 if causal else 0) + 1000003 * (max_dist or 0))
        lo = torch.zeros(n_q, dtype=torch.int64) if max_dist is None else (i - (max_dist - 1)).clamp(min=0)
        hi = i if causal else (i + max_dist - 1).clamp(max=n_k - 1)
        while True:                                          # seeded draws inside the allowed span, until the map is not trivial
            pi = lo + (torch.rand(n_q, generator=g, dtype=F64) * (hi - lo + 1).double()).long().clamp(max=n_k - 1)
            pi = torch.minimum(pi, hi)
            if causal and n_q > 2 and not bool((pi[1:] == i[1:]).any()):
                pi[n_q - 2] = n_q - 2
            if n_q <= 2 or not _trivial(pi, n_k):
                return pi
    if n_q == n_k and 3 <= n_k <= 6:                     # too few keys for a stride walk to differ between neighbours
        import itertools
        perms = [p for p in itertools.permutations(range(n_k)) if not _trivial(torch.tensor(p), n_k)]
        return torch.tensor(perms[(salt * 37) % len(perms)])
    step = max(1, int(0.38 * n_k) + salt % 5)
    while n_k > 1 and _gcd(step, n_k) != 1:
        step += 1
    pi = (i * step + 3 * salt + 1) % n_k
    if n_k - 1 not in pi.tolist():
        pi[(3 + salt) % n_q] = n_k - 1
    return pi


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def _dim_signs():
    """the sign of c in dim j, one pattern for every case, sequence and key/value set -- and for the accumulate base of an
    equal-weight case: terms that are normalised separately (c1 (1 + e1) + c2 (1 + e2) + base, e ~ 2^-24) then never sum to 0,
    the one value whose nearest bf16 number the e's could change"""
    return _signs(torch.Generator().manual_seed(20240), D)


def _sigma(g, n):
    """a zero-sum sequence of n signs in {+1, -1, 0} in seeded random order"""
    s = torch.cat([torch.ones(n // 2), -torch.ones(n // 2), torch.zeros(n % 2)]).double()
    return s[torch.randperm(n, generator=g)]


def _equal_v(g, n_seq, n_k, lim=7):
    """-> (v [n_seq, n_k, 64], c [n_seq, 64]): v[s, k, j] = c[s, j] + sigma_s[(k + r_sj) % n_k] d[s, j], r seeded per dim"""
    cc = _ints(g, 1, lim, n_seq, D) * _dim_signs()[None, :]
    dd = _ints(g, 1, lim, n_seq, D) * _signs(g, n_seq, D)
    k = torch.arange(n_k)[:, None]
    rows = []
    for s in range(n_seq):
        while True:                                          # a sign sequence with a rotational symmetry repeats rows: draw again
            vs = cc[s][None, :] + _sigma(g, n_k)[(k + torch.randint(0, n_k, (1, D), generator=g)) % n_k] * dd[s][None, :]
            if len({tuple(r.tolist()) for r in vs}) == n_k:
                break
        rows.append(vs)
    v = torch.stack(rows)
    return v, cc


# ------------------------------------------------------------------------------------------------- layouts <-> sequences
def rows_to_seq(x, batch, heads, n):
    """[batch * n, heads * 64] rows -> [batch * heads, n, 64]"""
    return x.reshape(batch, n, heads, D).permute(0, 2, 1, 3).reshape(batch * heads, n, D)


def seq_to_rows(x, batch, heads, n):
    return x.reshape(batch, heads, n, D).permute(0, 2, 1, 3).reshape(batch * n, heads * D)


def frames_to_seq(x, b, t, hw, heads):
    """[b * t * hw, heads * 64] with row = (clip * t + frame) * hw + pixel -> [(clip, pixel, head), t, 64]"""
    return x.reshape(b, t, hw, heads, D).permute(0, 2, 3, 1, 4).reshape(b * hw * heads, t, D)


def seq_to_frames(x, b, t, hw, heads):
    return x.reshape(b, hw, heads, t, D).permute(0, 3, 1, 2, 4).reshape(b * t * hw, heads * D)


def kv_index(c, bdiv, mod=False):
    """query batch -> K/V batch"""
    return [(b % bdiv if mod else b // bdiv) for b in range(c.batch)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(c):
    """Deterministic CPU tensors (float64, every value a bf16 number) in the operator's own layout, plus what the closed form
    and the report need: pi [n_seq, n_q] (gather), cvec [n_seq, 64] (equal), vseq [n_seq, n_k, 64] (the V rows a sequence sees),
    addend [rows, C] (what the operator adds to v[pi]).  A sequence is one (batch, head) / (clip, pixel, head)."""
    if c.spatial:
        return _spatial_inputs(c)
    if c.op in ("temporal", "temporal_rel"):
        return _temporal_inputs(c)
    return _fused_inputs(c)


def _spatial_inputs(c):
    g = _gen(c)
    heads, lq, batch = c.heads, c.lq, c.batch
    rows = batch * lq
    lim = 14 if c.op == "attention_q8" else 60
    dual = c.lk2 > 0
    amp = 16.0 if dual else 8.0
    inp = {}
    q = torch.zeros(batch * heads, lq, D, dtype=F64)
    if c.kind == "equal":
        q = _ints(g, -2, 2, batch * heads, lq, D)
    addend = torch.zeros(rows, heads * D, dtype=F64)
    for s, (lk, bdiv) in enumerate(((c.lk, c.kv_bdiv), (c.lk2, c.kv2_bdiv))[:2 if dual else 1]):
        kvb = (batch + bdiv - 1) // bdiv
        dims = slice(0, D) if not dual else slice(32 * s, 32 * s + 32)
        idx = torch.tensor([b // bdiv for b in range(batch)])
        seq_kv = (idx[:, None] * heads + torch.arange(heads)[None, :]).reshape(-1)      # sequence -> its (K/V batch, head)
        if c.kind == "gather":
            code = _signs(g, kvb * heads, lk, D)
            k = torch.zeros(kvb * heads, lk, D, dtype=F64)
            k[:, :, dims] = amp * code[:, :, dims]
            v = _ints(g, -lim, lim, kvb * heads, lk, D)
            pi = torch.stack([make_pi(lq, lk, 3 * b + 5 * h + 7 * s) for b in range(batch) for h in range(heads)])
            q[:, :, dims] = torch.gather(k[seq_kv], 1, pi[:, :, None].expand(-1, -1, D))[:, :, dims]
            picked = torch.gather(v[seq_kv], 1, pi[:, :, None].expand(-1, -1, D))
            inp["pi" if s == 0 else "pi2"] = pi
        else:
            kvec = _signs(g, kvb * heads, 1, D)
            k = kvec.expand(-1, lk, -1).clone()
            v, cc = _equal_v(g, kvb * heads, lk)
            picked = cc[seq_kv][:, None, :].expand(-1, lq, -1)
            inp["cvec" if s == 0 else "cvec2"] = cc[seq_kv]
        suffix = "" if s == 0 else "2"
        inp["k" + suffix], inp["v" + suffix] = seq_to_rows(k, kvb, heads, lk), seq_to_rows(v, kvb, heads, lk)
        if s == 0:
            inp["vseq"] = v[seq_kv]
            inp["picked"] = seq_to_rows(picked, batch, heads, lq)
        else:
            addend = addend + seq_to_rows(picked, batch, heads, lq)
    inp["q"] = seq_to_rows(q, batch, heads, lq)
    if c.accumulate:
        inp["base"] = _ints(g, -60, 60, rows, heads * D)
        if c.kind == "equal":                                # with the sign of c: no sum is zero (_dim_signs)
            inp["base"] = inp["base"].abs() * _dim_signs().repeat(heads)[None, :]
        addend = addend + inp["base"]
    inp["addend"] = addend
    return inp


def rel_index(c, n_q, n_k, defect=None):
    """idx[i, j] = clamp(j - i, -L, L) + L (attention_temporal_rel.hip, first line of its header)"""
    L = c.max_rel
    d = torch.arange(n_k)[None, :] - torch.arange(n_q)[:, None]
    idx = (d + L) % (2 * L + 1) if defect == "no_clamp" else d.clamp(-L, L) + L
    if defect == "rel_off1":
        idx = (idx + 1).clamp(max=2 * L)
    return idx


def _temporal_inputs(c):
    g = _gen(c)
    b, t, hw, heads = c.batch, c.t, c.hw, c.heads
    n = b * hw * heads
    inp = {}
    addend = torch.zeros(n, t, D, dtype=F64)
    if c.tables:
        L = c.max_rel
        inp["rel_k"] = torch.zeros(2 * L + 1, D, dtype=F64)
        inp["rel_v"] = torch.zeros(2 * L + 1, D, dtype=F64) if c.zero_tables else _ints(g, -40, 40, 2 * L + 1, D)
    if c.kind in ("gather", "gather_dist"):
        by_dist = c.kind == "gather_dist"
        pi = torch.stack([make_pi(t, t, s + s // heads, causal=c.causal, max_dist=(min(c.max_rel, t) if by_dist else None))
                          for s in range(n)])
        v = _ints(g, -60, 60, n, t, D)
        if by_dist:
            inp["rel_k"] = 8.0 * _signs(g, 2 * c.max_rel + 1, D)
            k = _signs(g, n, 1, D).expand(-1, t, -1).clone()
            q = inp["rel_k"][pi - torch.arange(t)[None, :] + c.max_rel]                  # the code of the target's distance
        else:
            k = 8.0 * _signs(g, n, t, D)
            q = torch.gather(k, 1, pi[:, :, None].expand(-1, -1, D))
        picked = torch.gather(v, 1, pi[:, :, None].expand(-1, -1, D))
        if c.tables:
            idx = (pi - torch.arange(t)[None, :]).clamp(-c.max_rel, c.max_rel) + c.max_rel
            addend = inp["rel_v"][idx]
        inp["pi"] = pi
    else:
        q = _ints(g, -2, 2, n, t, D)
        k = _signs(g, n, 1, D).expand(-1, t, -1).clone()
        v, cc = _equal_v(g, n, t)
        inp["cvec"] = cc
        picked = cc[:, None, :].expand(-1, t, -1)
    inp["qkv"] = torch.cat([seq_to_frames(x, b, t, hw, heads) for x in (q, k, v)], 1)
    inp["vseq"] = v
    inp["picked"] = seq_to_frames(picked, b, t, hw, heads)
    inp["addend"] = seq_to_frames(addend, b, t, hw, heads)
    return inp


def _fused_inputs(c):
    """x [b * t * hw, c] of +-1: column block 0 holds kappa(f) of the row's frame, block m >= 1 kappa(pi_m(f)) with one permutation
    pi_m per (clip, pixel, block).  Head h < heads - 1 takes its q from block h + 1 and its k from block 0 (target pi_{h+1}(f));
    the last head takes q from block 0 and k from block 1 (target: the INVERSE of pi_1).  wqkv's q / k rows select one column
    each, times +-8, through one signed permutation of the head's dims (the same for q and k: scores are unchanged); k gets an
    integer bias (q . bias is the same for every key); v[d] = 4 x[a] + 2 x[b] + x[c] + bias[d] with columns of block 0."""
    g = _gen(c)
    b, t, hw, heads = c.batch, c.t, c.hw, c.heads
    cw = heads * D
    npix = b * hw
    code = _signs(g, npix, t, D)                                                           # kappa of (clip, pixel), frame
    perms = torch.stack([torch.stack([torch.randperm(t, generator=g) for _ in range(heads)]) for _ in range(npix)])   # [npix, blocks, t]
    xs = torch.zeros(npix, t, cw, dtype=F64)
    xs[:, :, :D] = code
    for m in range(1, heads):
        xs[:, :, m * D:(m + 1) * D] = torch.gather(code, 1, perms[:, m][:, :, None].expand(-1, -1, D))
    x = xs.reshape(b, hw, t, cw).permute(0, 2, 1, 3).reshape(b * t * hw, cw)
    wqkv = torch.zeros(3 * cw, cw, dtype=F64)
    bqkv = torch.zeros(3 * cw, dtype=F64)
    pi = torch.zeros(npix, heads, t, dtype=torch.int64)
    for h in range(heads):
        qb, kb = (h + 1, 0) if h < heads - 1 else (0, 1)
        perm, sgn = torch.randperm(D, generator=g), _signs(g, D)
        for d in range(D):
            wqkv[h * D + d, qb * D + perm[d]] = 8.0 * sgn[d]
            wqkv[cw + h * D + d, kb * D + perm[d]] = 8.0 * sgn[d]
            cols = torch.randperm(D, generator=g)[:3]
            wqkv[2 * cw + h * D + d, cols] = torch.tensor([4.0, 2.0, 1.0], dtype=F64)
        pi[:, h] = perms[:, h + 1] if h < heads - 1 else torch.argsort(perms[:, 1], dim=1)
    bqkv[cw:2 * cw] = _ints(g, -1, 1, cw)
    bqkv[2 * cw:] = _ints(g, -20, 20, cw)
    v = xs[:, :, :D] @ wqkv[2 * cw:, :D].t() + bqkv[2 * cw:]                              # [npix, t, cw], integers
    vseq = v.reshape(npix, t, heads, D).permute(0, 2, 1, 3).reshape(npix * heads, t, D)
    pi = pi.reshape(npix * heads, t)
    picked = seq_to_frames(torch.gather(vseq, 1, pi[:, :, None].expand(-1, -1, D)), b, t, hw, heads)
    inp = dict(x=x, wqkv=wqkv, bqkv=bqkv, pi=pi, vseq=vseq, picked=picked, addend=torch.zeros_like(picked))
    if c.op == "tb_fused":
        wo = torch.zeros(cw, cw, dtype=F64)
        wo[torch.arange(cw), torch.randperm(cw, generator=g)] = _signs(g, cw)
        inp["wo"], inp["bo"] = wo, _ints(g, -20, 20, cw)
    return inp


# -------------------------------------------------------------------------------------------------------- expected values
def _swap_p(p):
    """keys +4..7 and +8..11 of every 16-key step exchanged"""
    n = p.shape[-1]
    pad = -n % 16
    pp = torch.nn.functional.pad(p, (0, pad))
    j = torch.arange(n + pad)
    r = j % 16
    src = torch.where((r >= 4) & (r < 8), j + 4, torch.where((r >= 8) & (r < 12), j - 4, j))
    return pp[..., src], pad


def _core(c, q, k, v, defect=None, rel=None, want_p=False):
    """q [S, n_q, 64], k, v [S, n_k, 64] (float64) -> o [S, n_q, 64]: softmax(q k^T / 8 [+ q Rk[idx]^T / 8]) (v [+ Rv[idx]]) with the
    family's rounding points (module docstring)."""
    S, n_k, _ = k.shape
    n_q = q.shape[1]
    if defect == "pad_key":
        k = torch.cat([k, torch.zeros(S, 1, D, dtype=F64)], 1)
        v = torch.cat([v, torch.zeros(S, 1, D, dtype=F64)], 1)
    n = k.shape[1]
    s = (q @ k.transpose(1, 2)) * SCALE
    i, j = torch.arange(n_q)[:, None], torch.arange(n)[None, :]
    vis = torch.ones(n_q, n, dtype=torch.bool)
    if c.causal:
        vis = (j < i) if defect == "causal_ge" else (j <= i)
    if defect == "drop_last" and n_k % c.tile:
        vis = vis.clone()
        vis[:, n_k - 1] = False
    idx = None
    if rel is not None:
        idx = rel_index(c, n_q, n, defect)
        s = s + SCALE * torch.gather(q @ rel[0].t(), 2, idx[None].expand(S, -1, -1))
    s = s.masked_fill(~vis[None], float("-inf"))
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    if want_p:
        return e / l
    if c.family == "flash":
        w = rne_bf16(e)                               # attn_tile64.h tc_tile64_pack_p: P = exp2(..) un-normalised, in bf16
    elif c.family == "mfma":
        w = rne_bf16(e / l)                           # attn_frames16.h / attn_frames_long.h: the NORMALISED weight in bf16
    else:
        w = e / l                                     # attention.hip attn_temporal_kernel: fp32 throughout
    wv = w
    if defect == "swap_p":
        wv, pad = _swap_p(w)
        v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    o = wv @ v
    if rel is not None:
        pb = torch.zeros(S, n_q, 2 * c.max_rel + 1, dtype=F64).scatter_add_(2, idx[None].expand(S, -1, -1), w)
        o = o + rne_bf16(pb) @ rel[1]                 # attention_temporal_rel.hip: "bf16 softmax weights and bucket sums"
    if c.family == "flash":
        o = o / l                                     # attn_tile64.h tc_tile64_store: O / l once
    return o


def _swap_heads(x, heads):
    """[..., heads * 64] with heads h and h + 1 exchanged (h even; an odd last head stays)"""
    order = []
    for h in range(0, heads - 1, 2):
        order += [h + 1, h]
    if heads % 2:
        order.append(heads - 1)
    return x.reshape(*x.shape[:-1], heads, D)[..., order, :].reshape(x.shape)


def project(c, inp):
    """the fused launches' q / k / v projection in float64 (exact integers): [rows, 3 c]"""
    return inp["x"] @ inp["wqkv"].t() + inp["bqkv"]


def expected(c, inp, defect=None, want_p=False):
    """The stored output (bf16 [rows, C]) by a float64 softmax with the kernel family's rounding points; `defect`: one of
    DEFECTS, seeded into the computation.  want_p: the float64 softmax weights [S, n_q, n_k] of the first key/value set."""
    heads = c.heads
    if c.spatial:
        q = rows_to_seq(inp["q"], c.batch, heads, c.lq)
        o = 0
        for sfx, lk, bdiv in (("", c.lk, c.kv_bdiv), ("2", c.lk2, c.kv2_bdiv))[:2 if c.lk2 else 1]:
            kvb = (c.batch + bdiv - 1) // bdiv
            v = _swap_heads(inp["v" + sfx], heads) if defect == "head_swap_v" else inp["v" + sfx]
            ks, vs = rows_to_seq(inp["k" + sfx], kvb, heads, lk), rows_to_seq(v, kvb, heads, lk)
            sel = (torch.tensor(kv_index(c, bdiv, mod=defect == "bdiv_mod"))[:, None] * heads + torch.arange(heads)[None, :]).reshape(-1)
            r = _core(c, q, ks[sel], vs[sel], defect, want_p=want_p)
            if want_p:
                return r
            o = o + r
        out = seq_to_rows(o, c.batch, heads, c.lq)
        if c.accumulate:
            out = out + inp["base"]
        out = out.float().to(BF16)
        if defect == "skip_row127":
            keep = inp["base"].float().to(BF16) if c.accumulate else torch.full_like(out, SENTINEL)
            rows = (torch.arange(c.batch * c.lq) % c.lq) % 128 == 127
            out[rows] = keep[rows]
        return out
    b, t, hw = c.batch, c.t, c.hw
    cw = heads * D
    qkv = inp["qkv"] if "qkv" in inp else project(c, inp)
    vcols = _swap_heads(qkv[:, 2 * cw:], heads) if defect == "head_swap_v" else qkv[:, 2 * cw:]
    q, k, v = (frames_to_seq(x, b, t, hw, heads) for x in (qkv[:, :cw], qkv[:, cw:2 * cw], vcols))
    rel = (inp["rel_k"], inp["rel_v"]) if c.tables else None
    o = _core(c, q, k, v, defect, rel=rel, want_p=want_p)
    if want_p:
        return o
    out = seq_to_frames(o, b, t, hw, heads)
    if c.op == "tb_fused":
        # tb_fused.hip: "Roundings: .. the attention output in bf16", then out = x + wo . a + bo in fp32, one bf16 store
        out = inp["x"] + rne_bf16(out) @ inp["wo"].t() + inp["bo"]
    return out.float().to(BF16)


def visible_keys(c):
    """n[i]: how many keys query i of a temporal case sees"""
    return torch.arange(1, c.t + 1) if c.causal else torch.full((c.t,), c.t)


def closed_form(c, inp):
    """The same stored output WITHOUT attention arithmetic: v[pi] + addend (gather), c (equal weights, un-normalised or fp32
    weights), rne_bf16(bf16(1 / n) * sum of the visible v) (equal weights on the MFMA cores)."""
    if c.kind != "equal":
        out = inp["picked"] + inp["addend"]
    elif c.family != "mfma":
        out = inp["picked"] + inp["addend"]
    else:
        n = visible_keys(c)
        w = rne_bf16(1.0 / n.double())                                                    # [t]
        v = inp["vseq"]                                                                   # [S, t, 64]
        sums = torch.cumsum(v, 1) if c.causal else v.sum(1, keepdim=True).expand(-1, c.t, -1)
        out = seq_to_frames(w[None, :, None] * sums, c.batch, c.t, c.hw, c.heads) + inp["addend"]
    if c.op == "tb_fused":
        out = inp["x"] + out @ inp["wo"].t() + inp["bo"]
    return out.float().to(BF16)


# ------------------------------------------------------------------------------------------------------------ validation
def _trivial(pi, n_k):
    i = torch.arange(pi.shape[0])
    return bool((pi == i).all()) or bool((pi[1:] >= pi[:-1]).all())


def validate(c, inp):
    """-> the list of violated conditions (module docstring); empty for a sound case"""
    bad = []
    n_q, n_k = (c.lq, c.lk) if c.spatial else (c.t, c.t)
    heads = c.heads
    vseq = inp["vseq"]
    if c.kind != "equal":
        p = expected(c, inp, want_p=True)
        pi = inp["pi"]
        w = torch.gather(p, 2, pi[:, :, None]).squeeze(2)
        if float((1 - w).max()) >= 2.0 ** -30:
            bad.append(f"gather mass: 1 - w_target up to {float((1 - w).max()):.3e}")
        if c.lk2:
            bad += ["second set's target map missing"] if "pi2" not in inp else []
        sums = [inp["picked"], inp["picked"] + inp["addend"]]
        if c.op == "tb_fused":
            sums.append(inp["x"] + (inp["picked"] @ inp["wo"].t()) + inp["bo"])
        if "base" in inp:
            sums.append(inp["addend"] - inp["base"] + inp["picked"])
        for x in sums:
            if not bool((x == x.round()).all()) or float(x.abs().max()) > 256:
                bad.append(f"an expected value or intermediate sum is no integer within +-256 (max {float(x.abs().max())})")
        # target maps
        if n_k > 2 and n_q > 2:
            for s in range(pi.shape[0]):
                if _trivial(pi[s], n_k):
                    bad.append(f"pi of sequence {s} is the identity or monotone")
                    break
            groups = pi.reshape(-1, heads, n_q)
            if heads > 1 and any(torch.equal(gp[h], gp[h + 1]) for gp in groups for h in range(heads - 1)):
                bad.append("two heads share a target map")
            if groups.shape[0] > 1 and any(torch.equal(groups[i][0], groups[i + 1][0]) for i in range(groups.shape[0] - 1)):
                bad.append("two batches / pixels share a target map")
        if c.kind == "gather":
            for s in range(pi.shape[0]):
                row = pi[s]
                want = min(n_q, n_k) if not c.causal else 0
                if len(set(row.tolist())) < want:
                    bad.append(f"pi of sequence {s} hits {len(set(row.tolist()))} keys where {want} are possible")
                    break
                if not c.causal and n_k - 1 not in row.tolist():
                    bad.append(f"pi of sequence {s} never hits the last valid key")
                    break
        if c.causal and not bool((pi <= torch.arange(n_q)[None, :]).all()):
            bad.append("a causal target lies behind its query")
        if c.causal and n_q > 2 and not bool((pi[:, 1:] == torch.arange(1, n_q)[None, :]).any()):
            bad.append("no causal query targets itself")
        if c.tables and c.kind == "gather" and c.max_rel < c.t - 1 and not bool(((pi - torch.arange(n_q)[None, :]).abs() > c.max_rel).any()):
            bad.append("no target in the clamped range")
        if c.kind == "gather_dist" and not bool(((pi - torch.arange(n_q)[None, :]).abs() < c.max_rel).all()):
            bad.append("a distance target lies in a clamped bucket")
    else:
        if c.family == "mfma" and midpoint_margin() <= 2.0 ** -20:
            bad.append("1 / n too close to a bf16 midpoint")
        cv = inp["cvec"]
        if bool((cv == 0).any()):
            bad.append("a zero in c")
        if cv.shape[0] > 1 and len({tuple(r.tolist()) for r in cv}) < (cv.shape[0] if not c.spatial else len({(b // c.kv_bdiv, h) for b in range(c.batch) for h in range(heads)})):
            bad.append("two heads / batches share c")
        final = inp["picked"] + inp["addend"]
        if c.family != "mfma" and (bool((final == 0).any()) or not bool((final == final.round()).all()) or float(final.abs().max()) > 256):
            # c (1 + e1) + c2 (1 + e2) + base with e ~ 2^-24: the nearest bf16 value is the integer sum -- unless that sum is 0
            bad.append("an equal-weight output is zero or no integer within +-256")
        valid = vseq.sum(1) if not c.causal else None
        if valid is not None and not torch.equal(valid, n_k * cv):
            bad.append("the signs do not sum to zero over the valid keys")
    if c.op == "attention_q8" and float(max(inp["v"].abs().max(), 0)) > 14:
        bad.append("|v| > 14 on the 8-bit kernel")
    # V rows
    for s in range(vseq.shape[0]):
        if len({tuple(r.tolist()) for r in vseq[s]}) < vseq.shape[1]:
            bad.append(f"two V rows of sequence {s} are equal")
            break
    if c.kind != "equal" and vseq.shape[0] > 1:
        flat = vseq.reshape(-1, D)
        distinct = len({tuple(r.tolist()) for r in flat})
        kvs = len({(b // c.kv_bdiv, h) for b in range(c.batch) for h in range(heads)}) if c.spatial else vseq.shape[0]
        if distinct < kvs * vseq.shape[1]:
            bad.append("V rows repeat across heads / batches")
    for name, x in inp.items():
        if name in ("pi", "pi2"):
            continue
        if not torch.equal(x.float().to(BF16).double(), x):
            bad.append(f"{name} holds values that are no bf16 numbers")
    return bad


# ------------------------------------------------------------------------------------------------------------- reporting
def _locate(c, row, col):
    """(batch, head, query, dim, pixel | None, sequence) of an output element"""
    h, d = col // D, col % D
    if c.spatial:
        b, i = row // c.lq, row % c.lq
        return b, h, i, d, None, b * c.heads + h
    p = row % c.hw
    f = (row // c.hw) % c.t
    b = row // (c.hw * c.t)
    return b, h, f, d, p, (b * c.hw + p) * c.heads + h


def differences(c, got, want, inp=None, limit=6):
    """None when got == want (signed zero is one value), else the report a failing kernel is debugged from: how many outputs
    differ, the first few (batch, head, query, dim, got, want), the residues of the differing queries modulo 32 and 128 and of
    their target keys modulo 4, 8, 16, 32 and 64, and, for a gather case, which key's V row the first differing rows DO equal."""
    g, w = got.float(), want.float()
    if g.shape != w.shape:
        return f"{c.name} [{c.target}]: shape {tuple(g.shape)} != {tuple(w.shape)}"
    if torch.equal(g, w):
        return None
    bad = (g != w) | torch.isnan(g)
    idx = bad.nonzero()
    first = []
    for r, q in idx[:limit].tolist():
        b, h, i, d, p, _ = _locate(c, r, q)
        first.append(f"({b}, {h}, {i}, {d}, {float(g[r, q])!r}, {float(w[r, q])!r})")
    cells = sorted({_locate(c, r, (q // D) * D)[:3] + (_locate(c, r, q)[5], r) for r, q in idx.tolist()})   # (b, h, query, seq, row)
    queries = torch.tensor([x[2] for x in cells])
    res = "; ".join(f"queries mod {m}: {sorted(set((queries % m).tolist()))[:16]}" for m in (32, 128))
    msg = (f"{c.name} [{c.target}]: {int(bad.sum())} of {g.numel()} outputs differ in {len(cells)} (row, head) cells; first "
           f"(batch, head, query, dim, got, want): {', '.join(first)}; {res}")
    if inp is not None and "pi" in inp and c.op != "tb_fused":
        keys = torch.tensor([int(inp["pi"][x[3], x[2]]) for x in cells])
        msg += "; " + "; ".join(f"target keys mod {m}: {sorted(set((keys % m).tolist()))[:16]}" for m in (4, 8, 16, 32, 64))
        found = []
        for b, h, i, s, r in cells[:limit]:
            row = got[r, h * D:(h + 1) * D].double() - inp["addend"][r, h * D:(h + 1) * D]
            hit = (inp["vseq"][s] == row[None, :]).all(1).nonzero().flatten().tolist()
            found.append(f"(batch {b}, head {h}, query {i}: wanted key {int(inp['pi'][s, i])}, got " +
                         (f"the V row of key {hit[0]})" if hit else "no V row of its sequence)"))
        msg += "; which key's V row the output equals: " + ", ".join(found)
    return msg


# ------------------------------------------------------------------------------------------------------------- the table
def _cases():
    out = []

    def add(name, op, kind, target, family, **kw):
        out.append(Case(name=name, op=op, kind=kind, target=target, family=family, **kw))

    # ---- attention.hip: attn_d64_dma_kernel<false> (the default) and, in a child process under TC_ATTN_STAGE=reg, attn_d64_kernel.
    # Blocks of 128 queries, key tiles of 64, double buffered: one key tile (1, 31, 64), a ragged second tile (65, 77), three and
    # four tiles (129, 200); a one-row query tail (129), a tail block of 1 / 33 rows, two query blocks (200)
    spatial = [dict(lq=1, lk=1, batch=1, heads=1), dict(lq=33, lk=31, batch=2, heads=2), dict(lq=128, lk=64, batch=1, heads=3),
               dict(lq=129, lk=65, batch=3, heads=2, kv_bdiv=2), dict(lq=200, lk=77, batch=3, heads=1, kv_bdiv=2, accumulate=True),
               dict(lq=129, lk=129, batch=2, heads=2, packed=True), dict(lq=200, lk=200, batch=1, heads=2),
               dict(lq=1, lk=200, batch=2, heads=1), dict(lq=128, lk=129, batch=1, heads=1)]
    for kind in ("gather", "equal"):
        for s in spatial:
            tag = f"{s['lq']}x{s['lk']}-b{s['batch']}h{s['heads']}" + ("-div2" if s.get("kv_bdiv") else "") + \
                  ("-acc" if s.get("accumulate") else "") + ("-packed" if s.get("packed") else "")
            add(f"attn-{kind}-{tag}", "attention", kind, "attn_d64_dma_kernel<false>", "flash", **s)
    # ---- the dual key/value instance: lk = 200 with lk2 = 77 shared by pairs of batches, independent target maps
    dual = dict(lq=129, lk=200, lk2=77, kv2_bdiv=2, batch=3, heads=2)
    add("attn-dual-gather", "attention", "gather", "attn_d64_dma_kernel<true>", "flash", **dual)
    add("attn-dual-equal", "attention", "equal", "attn_d64_dma_kernel<true>", "flash", **dual)
    add("attn-dual-gather-acc", "attention", "gather", "attn_d64_dma_kernel<true>", "flash", accumulate=True, **dual)
    # ---- attention_q8.hip: int8 Q K^T, MXFP8 P V
    for kind in ("gather", "equal"):
        for lq, lk in ((40, 40), (130, 65), (129, 257)):
            add(f"q8-{kind}-{lq}x{lk}", "attention_q8", kind, "attn_d64_q8_kernel", "flash", lq=lq, lk=lk, batch=2, heads=2)
    # ---- attention.hip attn_temporal_kernel (t <= 16, VALU, four sequences per block) and attention_temporal_long.hip
    for kind in ("gather", "equal"):
        for b, t, hw, heads in ((2, 3, 5, 3), (1, 16, 7, 2), (1, 1, 9, 1)):
            add(f"tvalu-{kind}-b{b}t{t}hw{hw}h{heads}", "temporal", kind, "attn_temporal_kernel", "valu", batch=b, t=t, hw=hw, heads=heads)
        for t in (17, 32, 33, 64):
            add(f"tlong-{kind}-t{t}", "temporal", kind, f"attn_temporal_long_kernel<{32 if t <= 32 else 64}>", "mfma", batch=2, t=t, hw=7, heads=2)
    # ---- attention_temporal_rel.hip
    for t in (6, 17, 33, 64):
        tt = 32 if t <= 32 else 64
        rel_t, mask_t = f"attn_temporal_rel_kernel<{tt}, {4 if tt == 32 else 2}, true>", f"attn_temporal_rel_kernel<{tt}, 4, false>"
        shape = dict(batch=2, t=t, hw=3, heads=2)
        for max_rel in (4, t):
            for causal in (False, True):
                tag = f"t{t}-L{max_rel}-{'causal' if causal else 'full'}"
                add(f"rel-key-{tag}", "temporal_rel", "gather", rel_t, "mfma", max_rel=max_rel, causal=causal, tables=True, **shape)
                add(f"rel-dist-{tag}", "temporal_rel", "gather_dist", rel_t, "mfma", max_rel=max_rel, causal=causal, tables=True, **shape)
        add(f"rel-equal-t{t}-causal", "temporal_rel", "equal", rel_t, "mfma", max_rel=4, causal=True, tables=True, zero_tables=True, **shape)
        add(f"rel-equal-t{t}-full", "temporal_rel", "equal", rel_t, "mfma", max_rel=t, causal=False, tables=True, zero_tables=True, **shape)
        add(f"mask-gather-t{t}", "temporal_rel", "gather", mask_t, "mfma", causal=True, **shape)
        add(f"mask-equal-t{t}", "temporal_rel", "equal", mask_t, "mfma", causal=True, **shape)
    # ---- qkv_attn.hip (16 frames) / qkv_attn_long.hip (17 .. 64), under TC_QKV_ATTN=2
    for t, hw in ((16, 8), (17, 4), (33, 2), (64, 2)):
        for heads in (2, 5):
            target = "qkv_attn_kernel" if t == 16 else f"qkv_attn_long_kernel<{32 if t <= 32 else 64}>"
            add(f"qkv-t{t}-hw{hw}-h{heads}", "qkv_attn", "gather", target, "mfma", batch=2, t=t, hw=hw, heads=heads)
    # ---- tb_fused.hip, under TC_TB_FUSED=1: its one shape family
    add("tb-fused", "tb_fused", "gather", "tb_fused_kernel", "mfma", batch=2, t=16, hw=8, heads=5)
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
REG_CASES = [c for c in CASES if c.op == "attention" and not c.lk2]          # the register-staged arm has no dual instance
