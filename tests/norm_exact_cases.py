"""The table behind tests/test_norm_exact_cpu.py (no GPU) and tests/test_gpu_norm_exact.py (MI355X): GroupNorm, LayerNorm and
row-softmax problems on which every output element of csrc/norm.hip is held to the final bf16 rounding.

The expectation is a float64 computation.  The kernels' fp32 arithmetic (v_rsq, v_rcp, v_exp, 1 / N) errs by about 1e-6
relative, three orders of magnitude below half a bf16 ulp (2^-9), so the only rounding that counts is the final store:

  * where the expectation is a bf16 value (families A and S)          torch.equal;
  * elsewhere   |got - ref| <= 1 bf16 ulp of |ref|, ELEMENTWISE (not relative to the tensor's scale); a faithful kernel
    is within 0.5 ulp, so the bound has a factor of two and nothing is tuned on the GPU.  Where ref is 0 the bound is 0.

Input families.  A "group" is a (sample, group) pair of GroupNorm and a row of LayerNorm; N is its element count.

  A  two-level.  Each group has its own non-zero integer mean m (distinct per group, |m| <= 100) and its own spread d in
     {1, 2, 4, 8} (d <= |m| / 4 or 1: the mean is never small beside the spread, so that whatever enters the variance
     around a wrong mean shows); its elements are m + d and m - d, exactly N / 2 of each, placed by a seeded draw.  gamma
     is an odd integer 1 .. 7 and beta an even integer |beta| <= 40 per channel (so that SiLU's exponential stays a
     normal fp32 number).  mean = m and var = d^2 exactly, so the output is the odd
     integer +-gamma[ch] + beta[ch] (eps moves it by < 1e-5 relative, far from any rounding tie): torch.equal.  With silu
     the bound is 1 ulp around the float64 SiLU of that integer.  Statistics of a wrong group, sample or row shift the
     result by a multiple of gamma / d or scale it by >= 2; a gamma or beta of a wrong channel changes the integer.
     (One shape of the table, 2 x 37 x 96, has an odd N = 111: there one element of every group sits AT m, the output is
     +-gamma sqrt(N / (N - 1)) + beta, no bf16 value, and the case falls under the 1-ulp rule around the float64 operator.)
  B  unit-sum probes (LB for LayerNorm).  Integers in +-[1, 100]; max(2, N / 16) elements per group are 0 ("probes", at seeded
     positions; the two seeds of a shape put them on disjoint positions, so every position is non-zero in one of them); a
     few non-zero elements are moved so that every group sums to exactly 1.  All partial sums the kernels form in fp32 are
     integers below 2^24 (validate()), exact in any order.  beta = 0, gamma in [0.5, 1.5].  A probe's output is
     -gamma rstd / N: a non-zero element v dropped from (counted twice in) the sum makes it 1 - v (1 + v) -- 0, negative or
     >= 2 -- and every probe of the group moves by >= 100 %.
  C  one spike.  x = 0 except one element H = 128 in most groups (one group in seven stays empty and must come out as
     exact zeros); gamma = 1, beta = 0.  Inside a group the zeros come out near -1 / sqrt(N - 1) and the spike near
     sqrt(N - 1).  The spike rotates over launches (c_plan) until every row and every channel has carried it.
  S  softmax: scores are 0 on a chosen set of k columns and -200 elsewhere; exp(-200) is 0 in fp32, so the row is exactly
     bf16(1 / k) on the set and 0 off it (recip_margin(): fl32(1 / k) (1 +- 2^-22) never straddles a bf16 tie).

gn_path() restates the host dispatch of groupnorm_impl / gn_geo / gn_chunking, so that the table can say which kernel
instance each shape reaches; norm_model() / softmax_model() are plain torch statements of the operators that take a
named defect (DEFECTS), for test_norm_exact_cpu.py.  Nothing here calls code under test or depends on tests/emu_ops.py."""
from dataclasses import dataclass
from functools import lru_cache

import torch

BF16 = torch.bfloat16
F64 = torch.float64
SENTINEL = 7.5                  # no expected output of any case: A gives integers, B / C / S stay clear of it
PAD_ROWS = 37
SPIKE = 128.0


# ------------------------------------------------------------------------------------------------ the host dispatch, restated
@dataclass(frozen=True)
class GnPath:
    kernel: str                 # gn_onepass<256,4> | gn_onepass<256,13> | three (gn_stats, gn_finalize, gn_apply)
    label: str                  # the row of the shape table
    vu: int                     # 8-channel vectors per one-pass unit
    rpp: int                    # rows per pass of the one-pass kernel
    slots: int                  # gn_geo
    rows_pp: int
    nchunks: int                # gn_chunking
    chunk_rows: int


def gn_path(samples, rows, c):
    cpg = c // 32
    u = cpg
    while u % 8:
        u += cpg
    vu, gu = u // 8, u // cpg
    vpr = c // 8
    slots = (vpr + 255) // 256
    vps = (vpr + slots - 1) // slots
    rows_pp = 1 if slots > 1 else max(1, 256 // vps)
    per_sample = max(1, 512 // samples)
    n = max(1, min(per_sample, (rows + 7) // 8))
    chunk_rows = (rows + n - 1) // n
    nchunks = (rows + chunk_rows - 1) // chunk_rows
    rpp = 256 // vu if vu <= 256 else 0
    kernel, label = "three", None
    if c % u == 0 and gu <= 4 and vu <= 64:
        nblk = (c // u) * samples
        nbytes = rows * vu * 16 * samples * (c // u)
        passes = (rows + rpp - 1) // rpp
        if nblk >= 128 or nbytes <= (4 << 20):
            if passes <= 4:
                kernel = label = "gn_onepass<256,4>"
            elif passes <= 13:
                kernel = label = "gn_onepass<256,13>"
        if label is None:
            label = "three: two slots" if slots > 1 else "three: slab too tall"
    else:
        label = "three: gu>4"
    return GnPath(kernel, label, vu, rpp, slots, rows_pp, nchunks, chunk_rows)


def ln_instance(c):
    """(NV, R): vectors per lane and rows per wave of layernorm_kernel"""
    return (1, 4) if c <= 512 else (2, 2) if c <= 1024 else (4, 1)


# ------------------------------------------------------------------------------------------------------------------ the table
# (samples, rows, C) -> the path it is declared to reach (test_norm_exact_cpu.py holds gn_path to it)
GN_SHAPES = (
    ((3, 70, 320), "gn_onepass<256,4>"),        # vu 5, rpp 51, ragged second pass
    ((2, 1000, 64), "gn_onepass<256,4>"),       # vu 1, all 4 vectors, ragged last
    ((5, 7, 960), "gn_onepass<256,4>"),         # vu 15, one idle thread, rows < rpp
    ((2, 9, 1280), "gn_onepass<256,4>"),
    ((2, 300, 320), "gn_onepass<256,13>"),
    ((1, 221, 960), "gn_onepass<256,13>"),      # exactly full
    ((1, 325, 2560), "gn_onepass<256,13>"),     # vu 10, exactly full
    ((2, 37, 96), "three: gu>4"),               # rows_pp 21 > chunk_rows 8, last chunk 5 rows
    ((1, 40, 32), "three: gu>4"),               # one channel per group
    ((2, 230, 960), "three: slab too tall"),    # rows_pp 2
    ((1, 700, 1280), "three: slab too tall"),   # rows_pp 1, 88 chunks > gn_finalize's lane stride 64, last chunk 4 rows
    ((1, 330, 2560), "three: two slots"),       # second slot partly filled
    ((1, 216, 4096), "three: two slots"),       # both slots full
)
LN_WIDTHS = (8, 64, 328, 512, 520, 1024, 1032, 1280, 2048)
LN_ROWS = (1, 5, 18, 33)
LN_MX_WIDTHS = (64, 320, 512, 1024, 1280, 2048)     # C % 32 == 0; 64 and 320 have 2 pad columns of scales
EPS = (1e-5, 1e-6)
ODD_N_SHAPE = "groupnorm-2x37x96"       # the one shape of the table with an odd N = rows * C / 32 (family A: see above)


@dataclass(frozen=True)
class Case:
    name: str
    op: str                     # groupnorm | layernorm
    family: str                 # A | B | C      (B on LayerNorm rows is the issue's LB)
    samples: int                # layernorm: 1
    rows: int
    c: int
    eps: float = 1e-5
    silu: bool = False
    seed: int = 0
    path: str = ""              # groupnorm: the declared path; layernorm: the kernel instance

    @property
    def ng(self):
        """groups per row"""
        return 32 if self.op == "groupnorm" else 1

    @property
    def geo(self):
        """(statistics samples, rows per sample, groups per row): a LayerNorm row is a sample of one row and one group"""
        return (self.samples, self.rows, 32) if self.op == "groupnorm" else (self.rows, 1, 1)

    @property
    def n(self):
        """elements per group"""
        return self.rows * (self.c // 32) if self.op == "groupnorm" else self.c

    @property
    def total_rows(self):
        return self.samples * self.rows

    @property
    def rule(self):
        return "equal" if self.family == "A" and not self.silu and self.n % 2 == 0 else "ulp"

    @property
    def shape_key(self):
        return f"{self.op}-{self.samples}x{self.rows}x{self.c}"


def _cases():
    out = []
    for i, ((s, r, c), path) in enumerate(GN_SHAPES):
        tag = f"gn-{s}x{r}x{c}"
        for silu in (False, True):
            for eps in EPS:
                out.append(Case(f"{tag}-A{'-silu' if silu else ''}-eps{eps:g}", "groupnorm", "A", s, r, c, eps, silu, 0, path))
        for seed in (0, 1):
            out.append(Case(f"{tag}-B-seed{seed}", "groupnorm", "B", s, r, c, EPS[seed], False, seed, path))
        out.append(Case(f"{tag}-C", "groupnorm", "C", s, r, c, EPS[i % 2], False, 0, path))
    for i, c in enumerate(LN_WIDTHS):
        nv, rr = ln_instance(c)
        for j, r in enumerate(LN_ROWS):
            tag, inst = f"ln-{r}x{c}", f"layernorm<{nv},{rr}>"
            for eps in EPS:
                out.append(Case(f"{tag}-A-eps{eps:g}", "layernorm", "A", 1, r, c, eps, False, 0, inst))
            for seed in (0, 1):
                out.append(Case(f"{tag}-LB-seed{seed}", "layernorm", "B", 1, r, c, EPS[seed], False, seed, inst))
            out.append(Case(f"{tag}-C", "layernorm", "C", 1, r, c, EPS[(i + j) % 2], False, 0, inst))
    return tuple(out)


CASES = _cases()


@dataclass(frozen=True)
class SCase:
    name: str
    kind: str                   # onehot | equal | causal
    rows: int
    n: int
    n_out: int = 0              # 0: n
    lds: int = 0                # 0: n
    ldo: int = 0                # 0: n_out
    causal_period: int = 0

    @property
    def dims(self):
        n_out = self.n_out or self.n
        return self.n, n_out, self.lds or self.n, self.ldo or n_out


def _scases():
    out = [SCase(f"sm-onehot-{n}", "onehot", n, n) for n in (1, 255, 256, 257, 2560)]
    out += [SCase(f"sm-equal-{n}", "equal", n, n) for n in (255, 256, 300, 2560)]
    out.append(SCase("sm-causal-77", "causal", 3 * 77, 80, causal_period=77))
    out.append(SCase("sm-strides-77", "equal", 77, 77, n_out=80, lds=88, ldo=96))
    out.append(SCase("sm-strides-257", "onehot", 257, 257, n_out=264, lds=260, ldo=272))
    out.append(SCase("sm-strides-causal-77", "causal", 3 * 77, 77, n_out=80, lds=88, ldo=96, causal_period=77))
    return tuple(out)


SCASES = _scases()


# ---------------------------------------------------------------------------------------------------------------- helpers
def _gen(key, salt=0):
    return torch.Generator().manual_seed((sum((i + 1) * ord(ch) for i, ch in enumerate(key)) * 64 + salt) % (2 ** 31))


def rne_bf16(x):
    """float64 -> the bf16 value (as float64), through fp32 like every store of the library"""
    return x.float().to(BF16).double()


def bf16_ulp(ref):
    """the bf16 ulp of |ref| (float64 tensor): 2^(floor(log2 |ref|) - 7), the exponent held at -126; 0 where ref is 0"""
    a = ref.abs()
    _, e = torch.frexp(a)                                   # a = m 2^e with m in [0.5, 1)
    u = torch.ldexp(torch.ones_like(a), (e - 1).clamp(min=-126) - 7)
    return torch.where(a == 0, torch.zeros_like(a), u)


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def to_groups(t, samples, rows, ng):
    """[samples * rows, C] -> [samples * ng, rows * cpg] (a copy): one line per group"""
    c = t.shape[1]
    return t.reshape(samples, rows, ng, c // ng).permute(0, 2, 1, 3).reshape(samples * ng, rows * (c // ng))


def from_groups(v, samples, rows, ng, c):
    return v.reshape(samples, ng, rows, c // ng).permute(0, 2, 1, 3).reshape(samples * rows, c)


def _ranks(u):
    """rank of every element inside its line"""
    return torch.argsort(torch.argsort(u, dim=1), dim=1)


# ----------------------------------------------------------------------------------------------------------------- inputs
def _inputs_a(c):
    s, r, ng = c.geo
    g, n = s * ng, c.n
    gen = _gen(c.shape_key + "A")
    rank = _ranks(torch.rand(g, n, generator=gen))
    pool = torch.cat([torch.arange(-100, 0), torch.arange(1, 101)])
    m = pool[torch.randperm(200, generator=gen)[:g]].double()
    d = (2 ** torch.randint(0, 4, (g,), generator=gen)).double()
    d = torch.minimum(d, 2 ** torch.floor(torch.log2((m.abs() / 4).clamp(min=1))))    # |m| >= 4 d wherever |m| >= 4
    sign = (rank < n // 2).double() - (rank >= n - n // 2).double()         # odd N: the middle rank sits at m
    x = from_groups(m[:, None] + sign * d[:, None], s, r, ng, c.c)
    gamma = (2 * torch.randint(0, 4, (c.c,), generator=gen) + 1).double()
    beta = (2 * torch.randint(-20, 21, (c.c,), generator=gen)).double()
    return dict(x=x, gamma=gamma, beta=beta, m=m, d=d, sign=from_groups(sign, s, r, ng, c.c))


def probe_mask(c):
    """[groups, N] bool: the probes of this seed; the two seeds of a shape share one rank field and take its two ends"""
    s, r, ng = c.geo
    n = c.n
    rank = _ranks(torch.rand(s * ng, n, generator=_gen(c.shape_key + "probes")))
    k = max(2, n // 16)
    return rank < k if c.seed == 0 else rank >= n - k


def _unit_sum(v, order):
    """move a few non-zero elements of the int64 line v (in the given order) so that it sums to 1: values stay in +-[1, 100]"""
    delta = 1 - int(v.sum())
    if delta == 0:
        return
    sgn = 1 if delta > 0 else -1
    cap = (100 * sgn - v[order]) * sgn                          # how far each may move towards sgn * 100
    cum = torch.cumsum(cap, 0)
    j = int(torch.searchsorted(cum, abs(delta)))
    assert j < len(order), "not enough room to reach a unit sum"
    v[order[:j]] = 100 * sgn
    rem = abs(delta) - (int(cum[j - 1]) if j else 0)
    new = int(v[order[j]]) + sgn * rem
    if new == 0:                    # a value may not become a probe: overshoot by one, and take it back from another element
        new = sgn
        for t in list(range(j)) + list(range(j + 1, len(order))):
            w = int(v[order[t]]) - sgn
            if w != 0 and abs(w) <= 100:
                v[order[t]] = w
                break
        else:
            raise AssertionError("no element can give one back")
    v[order[j]] = new


def _inputs_b(c):
    s, r, ng = c.geo
    g, n = s * ng, c.n
    gen = _gen(c.shape_key + "B", c.seed)
    v = torch.randint(1, 101, (g, n), generator=gen) * (torch.randint(0, 2, (g, n), generator=gen) * 2 - 1)
    probes = probe_mask(c)
    v[probes] = 0
    for i in range(g):
        nz = torch.nonzero(v[i]).flatten()
        _unit_sum(v[i], nz[torch.randperm(len(nz), generator=gen)])
    assert bool((v.sum(1) == 1).all()) and bool(((v == 0) == probes).all()) and int(v.abs().max()) <= 100
    x = from_groups(v.double(), s, r, ng, c.c)
    gamma = (0.5 + torch.rand(c.c, generator=gen)).float().double()
    return dict(x=x, gamma=gamma, beta=torch.zeros(c.c, dtype=F64))


def _c_spikes(c, k):
    """family C, statistics sample number k since the first launch (GroupNorm: launch * samples + sample; LayerNorm:
    launch * rows + row) -> per group of that sample (row, channel) of its spike, or None for an empty group.  Group g is
    empty when (g + k) % 7 == 5; its spike walks the rows and channels with j, the number of its non-empty turns so far"""
    out = []
    for g in range(c.ng):
        if (g + k) % 7 == 5:
            out.append(None)
            continue
        a = (5 - g) % 7
        j = k - (max(0, (k - a + 6) // 7))
        if c.op == "groupnorm":
            cpg = c.c // 32
            out.append(((j * 32 + g * 13 % 32) % c.rows, g * cpg + (j + 3 * g) % cpg))
        else:
            out.append((0, j * 37 % c.c))
    return out


@lru_cache(maxsize=None)
def c_plan(c):
    """family C: the launches, each a list over statistics samples of _c_spikes(); grown until every row and (GroupNorm, and
    the 33-row LayerNorm case of each width) every channel has carried the spike; the other LayerNorm cases run 8 launches"""
    s, r, _ = c.geo
    all_channels = c.op == "groupnorm" or c.rows == max(LN_ROWS)
    rows_seen, ch_seen, plan = set(), set(), []
    while True:
        launch = [_c_spikes(c, len(plan) * s + i) for i in range(s)]
        plan.append(launch)
        for i, spikes in enumerate(launch):
            for sp in spikes:
                if sp is not None:
                    rows_seen.add(sp[0] if c.op == "groupnorm" else i)
                    ch_seen.add(sp[1])
        assert len(plan) <= 200
        if len(rows_seen) == c.rows and (len(ch_seen) == c.c if all_channels else len(plan) >= 8):
            return tuple(tuple(tuple(sp) for sp in launch) for launch in plan)


def _inputs_c(c, launch, device):
    s, r, ng = c.geo
    pos = [(i * r + sp[0], sp[1]) for i, spikes in enumerate(c_plan(c)[launch]) for sp in spikes if sp is not None]
    x = torch.zeros(c.total_rows, c.c, dtype=F64, device=device)
    if pos:
        rr, cc = (torch.tensor(t, device=device) for t in zip(*pos))
        x[rr, cc] = SPIKE
    return dict(x=x, gamma=torch.ones(c.c, dtype=F64, device=device), beta=torch.zeros(c.c, dtype=F64, device=device))


def launches(c):
    return len(c_plan(c)) if c.family == "C" else 1


def inputs(c, launch=0, device="cpu"):
    """x [total_rows, C], gamma [C], beta [C] as float64 holding bf16 (x) and fp32 (gamma, beta) values.  Family C (many
    launches of a few spikes) is built on `device`, and norm_ref / differences work wherever their operands are"""
    return _inputs_a(c) if c.family == "A" else _inputs_b(c) if c.family == "B" else _inputs_c(c, launch, device)


# ------------------------------------------------------------------------------------------------------------ expectations
def norm_ref(c, inp):
    """the operator in float64: the two-pass definition, nothing of the kernels' structure"""
    s, r, ng = c.geo
    v = to_groups(inp["x"], s, r, ng)
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    y = from_groups((v - mean) / torch.sqrt(var + c.eps), s, r, ng, c.c) * inp["gamma"] + inp["beta"]
    return silu64(y) if c.silu else y


def closed_form(c, inp):
    """what the family's construction says the output is, without any norm arithmetic (eps = 0)"""
    s, r, ng = c.geo
    if c.family == "A":
        y = inp["sign"] * inp["gamma"] * (c.n / (c.n - c.n % 2)) ** 0.5 + inp["beta"]
        return silu64(y) if c.silu else y
    if c.family == "C":
        n = c.n
        has = to_groups(inp["x"], s, r, ng).sum(1, keepdim=True) > 0
        v = torch.where(to_groups(inp["x"], s, r, ng) > 0, (n - 1) ** 0.5, -1.0 / (n - 1) ** 0.5) * has
        return from_groups(v.double(), s, r, ng, c.c)
    raise ValueError("family B has no closed form: its probes are held to -gamma rstd / N by the CPU test")


def expected(c, inp):
    """float64 [total_rows, C]: family A, even N -> the closed form (a bf16 value, or its float64 SiLU); else norm_ref"""
    return closed_form(c, inp) if c.family == "A" and c.n % 2 == 0 else norm_ref(c, inp)


def validate(c, inp=None):
    """the conditions the case's exactness rests on -> list of violations"""
    bad = []
    s, r, ng = c.geo
    n = c.n
    if c.family == "A" and n % 2 and c.shape_key != ODD_N_SHAPE:
        bad.append("N is odd: no half / half split")
    if c.family == "B":
        if c.op == "groupnorm":
            p = gn_path(c.samples, c.rows, c.c)
            # one-pass: the whole group's sum is formed in fp32 (the squares are taken around the mean, not summed raw);
            # three launches: a chunk's sum and sum of squares; the chunks meet in fp64
            worst = n * 100 if p.kernel != "three" else p.chunk_rows * (c.c // 32) * 10 ** 4
        else:
            worst = n * 100                                     # two-pass in registers: only the plain sum must be exact
        if worst >= 2 ** 24:
            bad.append(f"a partial sum can reach {worst} >= 2^24")
    if inp is not None:
        x = inp["x"]
        if not torch.equal(rne_bf16(x), x):
            bad.append("x is not bf16")
        if not (torch.equal(inp["gamma"].float().double(), inp["gamma"]) and torch.equal(inp["beta"].float().double(), inp["beta"])):
            bad.append("gamma / beta are not fp32")
        v = to_groups(x, s, r, ng)
        if c.family == "A":
            m, d = inp["m"], inp["d"]
            if len(set(m.tolist())) != len(m) or bool((m == 0).any()) or float(m.abs().max()) > 100:
                bad.append("means are not distinct non-zero integers within 100")
            off = (v - m[:, None]).abs()
            if bool(((m.abs() >= 4) & (m.abs() < 4 * d)).any()) or bool(((m.abs() < 4) & (d != 1)).any()):
                bad.append("a spread above |m| / 4")
            if not bool(((off == d[:, None]).sum(1) == n - n % 2).all()) or not bool((v.sum(1) == m * n).all()):
                bad.append("a group is not m +- d, half of each (odd N: and one element at m)")
            y = inp["sign"] * inp["gamma"] + inp["beta"]
            if float(y.abs().max()) > 256 or bool((y == 0).any()) or not torch.equal(rne_bf16(y), y):
                bad.append("+-gamma + beta is not a non-zero bf16 integer")
        if c.family == "B":
            if not bool((v.sum(1) == 1).all()) or float(v.abs().max()) > 100 or not bool((v == v.round()).all()):
                bad.append("a group is not integers within 100 that sum to 1")
            if int((v == 0).sum(1).min()) < 2:
                bad.append("a group has fewer than 2 probes")
            if not torch.equal(v == 0, probe_mask(c)):
                bad.append("the zeros are not the probes")
        if c.family == "C":
            if int((v != 0).sum(1).max()) > 1 or not bool(((v == 0) | (v == SPIKE)).all()):
                bad.append("more than one spike in a group")
    return bad


# --------------------------------------------------------------------------------------------------------------- judging
def _where(c, rows, chans, limit=8):
    """the (sample, group) pairs -- rows for LayerNorm -- of the given elements"""
    if c.op == "groupnorm":
        cpg = c.c // 32
        pairs = sorted({(int(r) // c.rows, int(ch) // cpg) for r, ch in zip(rows.tolist(), chans.tolist())})
        return f"(sample, group): {pairs[:limit]}{' ..' if len(pairs) > limit else ''} ({len(pairs)} in all)"
    rr = sorted(set(rows.tolist()))
    return f"rows: {rr[:limit]}{' ..' if len(rr) > limit else ''} ({len(rr)} in all)"


def differences(c, out, want, rule=None, what=""):
    """out (bf16 or float64 [total_rows, C]) against the stored expectation under the case's rule -> None, or a report:
    kernel path, count, the first few (row, channel, got, want, error in ulps), the groups hit and residues of the rows and
    channels hit: a row tail, a vector or a group boundary shows in those"""
    rule = rule or c.rule
    head = f"{what}{c.name} [{c.path}], {rule}: "
    if tuple(out.shape) != tuple(want.shape):
        return head + f"shape {tuple(out.shape)}, expected {tuple(want.shape)}"
    got = out.double()
    want = want.to(got.device)
    if rule == "equal":
        bad = ~(got == rne_bf16(want))
    else:
        bad = ~((got - want).abs() <= bf16_ulp(want))           # a NaN fails
    nbad = int(bad.sum())
    if not nbad:
        return None
    idx = torch.nonzero(bad).cpu()
    rows, chans = idx[:, 0], idx[:, 1]
    got, want = got.cpu(), want.cpu()
    first = []
    for r, ch in idx[:6].tolist():
        u = float(bf16_ulp(want[r, ch]))
        err = f"{abs(float(got[r, ch]) - float(want[r, ch])) / u:.2f} ulp" if u else "want exact 0"
        first.append(f"(row {r}, ch {ch}: got {float(got[r, ch]):.6g}, want {float(want[r, ch]):.6g}, {err})")
    in_sample = rows % c.rows if c.op == "groupnorm" else rows
    return (head + f"{nbad} of {bad.numel()} outputs differ; first: {' '.join(first)}; {_where(c, rows, chans)}; "
            f"rows in sample, first / last: {int(in_sample.min())} / {int(in_sample.max())} of {c.rows}; "
            f"rows mod 4: {sorted(set((in_sample % 4).tolist()))}; channels / 8 mod 4: {sorted(set((chans // 8 % 4).tolist()))}; "
            f"channels mod 8: {sorted(set((chans % 8).tolist()))}")


def judge(c, buf, want, rule=None, what=""):
    """buf [total_rows + PAD_ROWS, C]: the output in its first rows, sentinels behind -> None or a report"""
    n = c.total_rows
    if tuple(buf.shape) != (n + PAD_ROWS, c.c):
        return f"{what}{c.name}: buffer shape {tuple(buf.shape)}"
    tail = buf[n:].double() != SENTINEL
    if bool(tail.any()):
        r = sorted(set(torch.nonzero(tail)[:, 0].tolist()))
        return f"{what}{c.name} [{c.path}]: rows behind the output were written: output rows + {r[:8]}"
    return differences(c, buf[:n], want, rule, what)


# ------------------------------------------------------------------------------------ the operators with a seeded defect
# defect -> (operators it concerns, the family that must flag it)
DEFECTS = {
    "drop_chunk_last_row": (("groupnorm",), "B"),       # the last row of every chunk (one-pass: of the slab) not in the sums
    "drop_vector": (("groupnorm", "layernorm"), "B"),   # one 8-channel vector not in the sums
    "double_count": (("groupnorm", "layernorm"), "B"),  # one element counted twice
    "stats_next_group": (("groupnorm",), "A"),          # apply with the statistics of group g + 1
    "stats_next_sample": (("groupnorm", "layernorm"), "A"),    # ... of sample s + 1 / of row r + 1
    "gamma_shift8": (("groupnorm", "layernorm"), "A"),  # gamma of channel + 8
    "beta_shift8": (("groupnorm", "layernorm"), "A"),
    "pad_in_var": (("groupnorm", "layernorm"), "A"),    # padded rows (one-pass) / padded lanes (LayerNorm) in the variance sweep
    "spike_not_in_var": (("groupnorm", "layernorm"), "C"),     # the last row / vector missed by the variance sweep alone
    "store_past_tail": (("groupnorm", "layernorm"), "A"),      # the row behind the last one stored (a clamped row, a ragged pass)
}
S_DEFECTS = {
    "max_miss_last_stride": "onehot",   # the max reduction stops before the last, partial stride of 256 columns
    "sum_miss_col": "equal",            # the sum misses the last column
    "causal_off_by_one": "causal",      # row r sees r % period columns
    "pad_not_zeroed": "strides",        # columns [n, n_out) left as they were
    "store_past_tail": "strides",       # column n_out written
}


def pad_elements(c):
    """elements per group that the kernel holds as padding (zeros in registers) beside the N real ones"""
    if c.op == "layernorm":
        return ln_instance(c.c)[0] * 512 - c.c
    p = gn_path(c.samples, c.rows, c.c)
    if p.kernel == "three":
        return 0
    nv = 4 if p.kernel.endswith(",4>") else 13
    return (nv * p.rpp - c.rows) * (c.c // 32)


def occurs(defect, c):
    """can this defect change anything on this case's shape?"""
    if c.op not in DEFECTS[defect][0]:
        return False
    if defect == "stats_next_sample":
        return c.geo[0] > 1
    if defect in ("gamma_shift8", "beta_shift8"):
        return c.c > 8
    if defect == "pad_in_var":
        return pad_elements(c) > 0
    if defect == "spike_not_in_var":
        return c.n > 8
    return True


def norm_model(c, inp, defect=None):
    """GroupNorm / LayerNorm as the kernels build them (sums over chunks, E[x^2] - mean^2 on the three-launch path, squares
    around the mean elsewhere, count = the nominal N), in float64, with one named defect -> the whole output buffer
    [total_rows + PAD_ROWS, C] (float64; sentinels behind the output)"""
    s, r, ng = c.geo
    cpg, n = c.c // ng, c.n
    x = inp["x"]
    three = c.op == "groupnorm" and gn_path(c.samples, c.rows, c.c).kernel == "three"
    w = torch.ones(r, c.c, dtype=F64)                           # how often an element enters the sums
    wv = None                                                   # ... the variance sweep, where it differs
    if defect == "drop_chunk_last_row":
        ch = gn_path(c.samples, c.rows, c.c).chunk_rows if three else r
        w[[min(r0 + ch, r) - 1 for r0 in range(0, r, ch)]] = 0
    elif defect == "drop_vector":
        v = (c.c // 8) // 2
        w[:, 8 * v:8 * v + 8] = 0
    elif defect == "double_count":
        w[r - 1, c.c - 3] = 2
    elif defect == "spike_not_in_var":
        wv = w.clone()
        if c.op == "groupnorm":
            wv[r - 1] = 0
        else:
            wv[:, c.c - 8:] = 0
    wg = to_groups(w.repeat(s, 1), s, r, ng)
    v = to_groups(x, s, r, ng)
    mean = (wg * v).sum(1, keepdim=True) / n
    if three and wv is None:
        var = ((wg * v * v).sum(1, keepdim=True) / n - mean * mean).clamp(min=0)
    else:
        wq = wg if wv is None else to_groups(wv.repeat(s, 1), s, r, ng)
        q = (wq * (v - mean) ** 2).sum(1, keepdim=True)
        if defect == "pad_in_var":
            q = q + pad_elements(c) * mean * mean
        var = q / n
    rstd = 1.0 / torch.sqrt(var + c.eps)
    if defect == "stats_next_group":
        mean, rstd = (t.reshape(s, ng).roll(-1, 1).reshape(-1, 1) for t in (mean, rstd))
    elif defect == "stats_next_sample":
        mean, rstd = (t.reshape(s, ng).roll(-1, 0).reshape(-1, 1) for t in (mean, rstd))
    gamma = inp["gamma"].roll(-8) if defect == "gamma_shift8" else inp["gamma"]
    beta = inp["beta"].roll(-8) if defect == "beta_shift8" else inp["beta"]
    y = from_groups((v - mean) * rstd, s, r, ng, c.c) * gamma + beta
    if c.silu:
        y = silu64(y)
    buf = torch.full((c.total_rows + PAD_ROWS, c.c), SENTINEL, dtype=F64)
    buf[:c.total_rows] = rne_bf16(y)
    if defect == "store_past_tail":
        buf[c.total_rows] = buf[c.total_rows - 1]
    return buf


def gn_from_part(c, inp, part, prows):
    """tc_groupnorm_part in float64: statistics from per-block partial sums part [samples * rows / prows, 2, C]"""
    s, r, ng = c.geo
    cpg, n = c.c // 32, c.n
    p = part.double().reshape(s, r // prows, 2, 32, cpg).sum((1, 4))         # [s, 2, 32]
    mean = (p[:, 0] / n).reshape(-1, 1)
    var = ((p[:, 1] / n).reshape(-1, 1) - mean * mean).clamp(min=0)
    v = to_groups(inp["x"], s, r, ng)
    y = from_groups((v - mean) / torch.sqrt(var + c.eps), s, r, ng, c.c) * inp["gamma"] + inp["beta"]
    return silu64(y) if c.silu else y


def exact_part(x, prows):
    """the partial sums a producer would emit for x [rows, C]: [rows / prows, 2, C] fp32 (exact for family-B inputs)"""
    rows, c = x.shape
    b = x.reshape(rows // prows, prows, c)
    part = torch.stack([b.sum(1), (b * b).sum(1)], 1)
    assert float(part.abs().max()) < 2 ** 24
    return part.float()


PART_CASES = (          # tc_groupnorm_part: 300 row blocks (> gn_finalize_part's 256 threads), and one block per sample
    (Case("gn-part-2x600x64-prows2", "groupnorm", "B", 2, 600, 64, 1e-5, False, 0, "gn_finalize_part"), 2),
    (Case("gn-part-2x600x64-prows600", "groupnorm", "B", 2, 600, 64, 1e-6, False, 1, "gn_finalize_part"), 600),
)


# ---------------------------------------------------------------------------------------------------------------- softmax
NEG = -200.0
POISON = 1000.0                 # in the score columns [n, lds): a kernel that reads them gets a wrong max


def _s_set(c, r):
    """the columns of row r that carry score 0"""
    if c.kind == "onehot":
        return [r % c.n]
    k = 2 + r % 63
    cols = [(r + 257 * j) % c.n for j in range(k)]
    assert len(set(cols)) == k, (c.name, r)
    return cols


def s_inputs(c):
    """fp32 scores [rows, lds]"""
    n, n_out, lds, ldo = c.dims
    s = torch.full((c.rows, lds), POISON, dtype=torch.float32)
    if c.kind == "causal":
        s[:, :n] = 0.0
        return s
    s[:, :n] = NEG
    for r in range(c.rows):
        s[r, _s_set(c, r)] = 0.0
    return s


def s_closed_form(c):
    """the whole output buffer [rows + PAD_ROWS, ldo] as float64: bf16(1 / k) on each row's set, zeros in the rest of
    [0, n_out), sentinels beside and behind"""
    n, n_out, lds, ldo = c.dims
    buf = torch.full((c.rows + PAD_ROWS, ldo), SENTINEL, dtype=F64)
    buf[:c.rows, :n_out] = 0.0
    for r in range(c.rows):
        if c.kind == "causal":
            k = min(n, r % c.causal_period + 1)
            buf[r, :k] = 1.0 / k
        else:
            cols = _s_set(c, r)
            buf[r, cols] = 1.0 / len(cols)
    buf[:c.rows, :n_out] = rne_bf16(buf[:c.rows, :n_out])
    return buf


def softmax_model(c, s, defect=None):
    """softmax_rows_kernel in plain fp32 torch (max, exp, sum, reciprocal, product), with one named defect -> the buffer"""
    n, n_out, lds, ldo = c.dims
    buf = torch.full((c.rows + PAD_ROWS, ldo), SENTINEL, dtype=F64)
    for r in range(c.rows):
        k = n
        if c.causal_period:
            k = min(n, r % c.causal_period + 1 - (1 if defect == "causal_off_by_one" else 0))
        row = s[r, :k]
        kmax = (k - 1) // 256 * 256 if defect == "max_miss_last_stride" else k
        mx = torch.cat([row[:kmax], torch.tensor([-1e30])]).max()
        e = torch.exp(row - mx)
        inv = 1.0 / (e[:k - 1] if defect == "sum_miss_col" else e).sum()
        out = torch.zeros(n_out, dtype=torch.float32)
        out[:k] = e * inv
        hi = n if defect == "pad_not_zeroed" else n_out
        buf[r, :k] = rne_bf16(out[:k].double())
        buf[r, k:hi] = 0.0
        if defect == "store_past_tail" and n_out < ldo:
            buf[r, n_out] = 0.0
    return buf


def s_judge(c, buf, want=None):
    """the whole buffer against the closed form, bit for bit -> None or a report"""
    want = s_closed_form(c) if want is None else want
    got = buf.double().cpu()
    if tuple(got.shape) != tuple(want.shape):
        return f"{c.name}: buffer shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    bad = ~(got == want)
    if not bool(bad.any()):
        return None
    n, n_out, lds, ldo = c.dims
    idx = torch.nonzero(bad)
    first = [f"(row {r}, col {j}: got {float(got[r, j]):.6g}, want {float(want[r, j]):.6g})" for r, j in idx[:6].tolist()]
    cols = idx[:, 1]
    zone = [name for name, m in (("softmax columns [0, n)", cols < n), ("zero padding [n, n_out)", (cols >= n) & (cols < n_out)),
                                 ("sentinel columns [n_out, ldo)", cols >= n_out)) if bool((m & (idx[:, 0] < c.rows)).any())]
    if bool((idx[:, 0] >= c.rows).any()):
        zone.append("sentinel rows behind the output")
    return (f"{c.name} [softmax_rows] n {n} n_out {n_out} lds {lds} ldo {ldo}: {len(idx)} elements differ in {zone}; first: "
            f"{' '.join(first)}; columns mod 256: {sorted(set((cols % 256).tolist()))[:16]}")


def recip_margin(k_max=2560):
    """min over k = 1 .. k_max of the relative distance of fl32(1 / k) from the nearest bf16 rounding tie"""
    k = torch.arange(1, k_max + 1, dtype=F64)
    x = (1.0 / k).float().double()
    _, e = torch.frexp(x)
    ulp = torch.ldexp(torch.ones_like(x), e - 1 - 7)
    frac = torch.remainder(x / ulp, 1.0)
    return float(((frac - 0.5).abs() * ulp / x).min())
