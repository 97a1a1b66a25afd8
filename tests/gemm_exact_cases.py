"""The table behind tests/test_gemm_exact_cpu.py (no GPU) and tests/test_gpu_gemm_exact.py (MI355X): problems on which the
correct output of a GEMM kernel is known TO THE BIT, one or more per kernel instance of the family.

Why integers.  Products of bf16 integers are exact; fp32 accumulation is exact in ANY order while every partial sum stays
below 2^24; an integer of magnitude <= 256 is a bf16 value.  So with A in {-1, 0, 1}, W in {-1, +1} (or mirrored) and
epilogue operands that are small integers, "every product counted exactly once, every epilogue operand taken from the right
row and column, one correct rounding" is torch.equal against a float64 reference -- no tolerance for a dropped K-step of one
fragment, a tap decoded wrongly for one border lane or a truncating store to hide in.

What a case is: a problem (linear / conv 3x3 / conv T3, geometry, batch, epilogue operands, out_f32), a setting of the
routing switches (csrc/gemm_route.cpp), and the NAME of the kernel instance that setting sends the problem to, spelled as
tests/gemm_route_host_check.cpp prints it; test_gemm_exact_cpu.py runs the route and holds the table to that name, and to
covering every instance of tests/golden/gemm_routes.json.

Conditions every case meets by construction (asserted on the CPU, from the reference alone):
  * K max|a| max|w| + |epilogue terms| < 2^24;
  * non-rounding cases: EVERY output is sensitive.  With d = the smallest change one dropped or doubled product causes
    (|alpha out_scale|, x 8 in GEGLU pass (b), x the block scales' 2^e on the MXFP8 cases) and u = min(d, 1) (the epilogue
    operands are integers; 8 in GEGLU pass (b), where they are multiplied by the gate too), V / u is an integer and |V| + d < 256 u: V is a bf16 value, and so is V +- d, a different one.
    (For d <= 1 this reads |V| + d < 256 d; for d = 2, u = 1 is the stricter of the two readings, and the one that is true.)
  * rounding cases: a bias of 384 puts the outputs into 256..512, where bf16 steps by 2 and every odd integer is an exact tie:
    round-half-up, truncation and round-to-nearest-even all differ there.

GEGLU.  gelu_erf_f(x) (csrc/common.h) is fma(-|x|, poly e, max(x, 0)) with e = exp2(-0.72 x^2) and poly < 0.5.  For x >= 8
the subtracted term is below 8 * 0.5 * 2^-46 < 2^-40 while half an ulp of x in [8, 256) is at least 2^-21, so the fma returns
x: gelu(x) == x exactly.  A GEGLU case therefore runs as two passes over the packed weights (lvdm.common.pack_geglu):
  (a) value half pinned: its weight rows are zero, its bias 1; the gate bias lifts every gate pre-activation to an integer in
      [8, 255]; expected output = 1 * gate;
  (b) gate half pinned: its weight rows are zero, its bias 8, gelu(8) = 8; expected output = 8 v with |8 v| < 2048 (the
      bf16 significand of 8 v is that of v).

Not in the table: the three gemm_ws_kernel<..., true> instances (LayerNorm prologue): their rsqrtf (csrc/gemm_ws.hip, the a_norm prologue) is not exact on integers;
tests/test_gpu_gemm_ws.py keeps covering them against the emulation.

Adding a kernel instance: add a Case whose `target` is its name and whose `env` routes there; test_gemm_exact_cpu.py fails
(union check) until one exists."""
import os
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
ACT_NONE, ACT_GEGLU = 0, 3                 # tooncrafter_amd._lib (include/tooncrafter_hip.h); the GPU test asserts they agree
SENTINEL = 7.0                             # what the wider buffers of a strided case are filled with
EXEMPT = {f"gemm_ws_kernel<{v}, true>" for v in ("4, true, false", "5, false, true", "5, false, false")}
MX_TARGETS = {f"gemm_mx_kernel<{g}, {t}, {t}>" for g in range(3) for t in (1, 2)}


class env:
    """The library reads its tuning switches per call."""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@dataclass(frozen=True)
class Case:
    name: str
    target: str                 # the kernel instance, as tests/gemm_route_host_check.cpp prints it
    kind: str                   # lin | 3x3 | s2 | up | pad0 | t3  (3x3 flavours: stride 1, stride 2, nearest x2, trailing pad)
    n: int
    m: int = 0                  # lin
    k: int = 0                  # lin (convolutions: 9 cin / 3 cin)
    frames: int = 0             # conv
    h: int = 0                  # conv 3x3: SOURCE height (t3: unused)
    w: int = 0                  # conv 3x3: SOURCE width; t3: h * w of a frame
    cin: int = 0
    t_len: int = 16
    env: dict = field(default_factory=dict)
    args: str = ""              # the scalar arguments the route must hand over ("" = not pinned)
    also: tuple = ()            # further kernels the launch runs (splitk_reduce_kernel)
    bias: bool = True
    row_bias: bool = False
    residual: bool = False
    alpha: float = 1.0
    out_scale: float = 1.0
    out_f32: bool = False
    geglu: str = ""             # "" | "a" | "b": the pass (see the module docstring)
    batch: int = 1
    mirrored: bool = False      # A dense +-1, W sparse: W's K positions are the ones that thin out
    rounding: bool = False
    strided: bool = False       # A, residual and the output are column slices of wider, sentinel-filled buffers
    ldw: int = 0                # > k: W is a column slice of a wider buffer (the chunked walk prices n * ldw)
    mx: bool = False            # through the MXFP8 route (HipOps.fp8 = "all")
    mx_rc: bool = True          # MXFP8: the block scales also depend on the row / column (off for the rounding case)
    gn_stats: bool = False      # the call asks for GroupNorm partials (gemm16 stats instances); the OUTPUT is what is checked
    p: float = 0.5              # density of the sparse operand


def geometry(c):
    """-> dict(m, k, kc (columns of A), src_rows, row_div, conv (HipOps.gemm's dict | None), h_out, w_out)"""
    if c.kind == "lin":
        return dict(m=c.m, k=c.k, kc=c.k, src_rows=c.m, row_div=50, conv=None, h_out=0, w_out=0)
    if c.kind == "t3":
        conv = dict(kind="t3", frames=c.frames, t_len=c.t_len, cin=c.cin, h_out=1, w_out=c.w)
        return dict(m=c.frames * c.w, k=3 * c.cin, kc=c.cin, src_rows=c.frames * c.w, row_div=c.w, conv=conv, h_out=1, w_out=c.w)
    stride, ups, pad = (2, False, 1) if c.kind == "s2" else (2, False, 0) if c.kind == "pad0" else (1, c.kind == "up", 1)
    hv, wv = (2 * c.h, 2 * c.w) if ups else (c.h, c.w)
    extra = 2 if pad == 1 else 1
    ho, wo = (hv + extra - 3) // stride + 1, (wv + extra - 3) // stride + 1
    conv = dict(kind="3x3", frames=c.frames, cin=c.cin, h_in=c.h, w_in=c.w, h_out=ho, w_out=wo, stride=stride, upsample=ups, pad=pad)
    return dict(m=c.frames * ho * wo, k=9 * c.cin, kc=c.cin, src_rows=c.frames * c.h * c.w, row_div=ho * wo, conv=conv, h_out=ho, w_out=wo)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _seed(c, salt):
    return (sum((i + 1) * ord(ch) for i, ch in enumerate(c.name)) * 16 + salt) % (2 ** 31)


def _signs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _sparse(shape, seed, p):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(shape, generator=g, dtype=torch.float64) < p
    return _signs(shape, seed + 7919) * keep


def _pattern(rows, cols, mod, shift=0):
    """small integers that differ in every row AND column: (3 row + col + shift) mod `mod`, centred"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    q = torch.arange(cols, dtype=torch.int64)[None, :]
    return ((3 * r + q + shift) % mod - mod // 2).double()


def _mx_row_group(c, rows, output):
    """MXFP8 cases: what a row's exponent g may depend on so that every product of ONE output carries the same g: the row
    itself (linear), the frame (3x3: taps stay inside a frame), the clip (T3: taps cross frames).  `output`: rows of C, not of A."""
    r = torch.arange(rows)
    if c.kind == "lin":
        return r
    if c.kind == "t3":
        return r // (c.t_len * c.w)
    g = geometry(c)
    return r // (g["h_out"] * g["w_out"] if output else c.h * c.w)


def mx_exponents(c, rows, cols, kc, k, output=False):
    """MXFP8 cases: per-32-block powers of two, e_a[row, block] = g(row) + f(block), e_w[col, block] = h(col) - f(block) with
    f in [-2, 2], g, h in {-1, 0} (all within 2^-3..2^3).  f cancels in every product, so an output is an integer multiple of
    d[row, col] = 2^(g + h) -- a scale byte taken from the wrong block, row or column breaks that."""
    fa = (torch.arange(kc // 32) * 2 % 5 - 2)
    fw = (torch.arange(k // 32) % (kc // 32) * 2 % 5 - 2)                 # a convolution's taps see the same channel blocks
    g = -(_mx_row_group(c, rows, output) % 2) if c.mx_rc else torch.zeros(rows, dtype=torch.int64)
    h = -(torch.arange(cols) // 2 % 2) if c.mx_rc else torch.zeros(cols, dtype=torch.int64)
    return g[:, None] + fa[None, :], h[:, None] - fw[None, :], g, h


def inputs(c):
    """Deterministic CPU tensors (float64, every value a bf16 number): a [batch * src_rows, kc], w [batch * n, k] (GEGLU:
    UNPACKED, value rows then gate rows), bias [n] | None, row_bias [groups, n] | None, residual [batch * m, n_out] | None."""
    g = geometry(c)
    rows, n, k, kc = c.batch * g["src_rows"], c.n, g["k"], g["kc"]
    if c.mirrored:
        a, w = _signs((rows, kc), _seed(c, 1)), _sparse((c.batch * n, k), _seed(c, 2), c.p)
    else:
        a, w = _sparse((rows, kc), _seed(c, 1), c.p), _signs((c.batch * n, k), _seed(c, 2))
    n_out = n // 2 if c.geglu else n
    bias = _pattern(1, n, 7, 2)[0] if c.bias else None
    if c.rounding:
        bias = bias + 384.0
    if c.geglu == "a":
        w[:n_out] = 0
        bias[:n_out] = 1.0
        bias[n_out:] += 0.0 if c.rounding else 100.0
    elif c.geglu == "b":
        w[n_out:] = 0
        bias[n_out:] = 8.0
    if c.mx:
        ea, ew, _, _ = mx_exponents(c, rows, n, kc, k)
        a = a * torch.exp2(ea.double()).repeat_interleave(32, 1)
        w = w * torch.exp2(ew.double()).repeat_interleave(32, 1)
    groups = (g["m"] + g["row_div"] - 1) // g["row_div"]
    row_bias = _pattern(groups, n, 5, 1) if c.row_bias else None
    residual = _pattern(c.batch * g["m"], n_out, 7) if c.residual else None
    return dict(a=a, w=w, bias=bias, row_bias=row_bias, residual=residual)


# ------------------------------------------------------------------------------------------------------------- reference
def _acc(c, g, a, w, dt):
    """gather(a) @ w^T for one batch item, in dtype dt, by torch's own operators"""
    a, w = a.to(dt), w.to(dt)
    if c.kind == "lin":
        return a @ w.t()
    if c.kind == "t3":
        b, hw = c.frames // c.t_len, c.w
        x = a.reshape(b, c.t_len, hw, c.cin).permute(0, 3, 1, 2).unsqueeze(-1)              # [b, cin, t, hw, 1]
        wt = w.reshape(c.n, 3, c.cin).permute(0, 2, 1).reshape(c.n, c.cin, 3, 1, 1)        # K index = kt * cin + ci
        y = F.conv3d(x, wt, padding=(1, 0, 0))
        return y.squeeze(-1).permute(0, 2, 3, 1).reshape(g["m"], c.n)
    x = a.reshape(c.frames, c.h, c.w, c.cin).permute(0, 3, 1, 2)
    wt = w.reshape(c.n, 3, 3, c.cin).permute(0, 3, 1, 2)                                    # K index = (ky * 3 + kx) * cin + ci
    if c.kind == "up":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if c.kind == "pad0":
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, stride=2)
    else:
        y = F.conv2d(x, wt, stride=2 if c.kind == "s2" else 1, padding=1)
    return y.permute(0, 2, 3, 1).reshape(g["m"], c.n)


def reference(c, inp, dt=torch.float64, acc_hook=None, bias=None):
    """-> V [batch * m, n_out], the value before the ONE rounding of the store, in dtype dt.  acc_hook(acc, item) may edit the
    products' sum and `bias` replace the bias (the seeded defects of test_gemm_exact_cpu.py)."""
    g = geometry(c)
    m, n, sr = g["m"], c.n, g["src_rows"]
    bias = inp["bias"] if bias is None else bias
    out = []
    for z in range(c.batch):
        acc = _acc(c, g, inp["a"][z * sr:(z + 1) * sr], inp["w"][z * n:(z + 1) * n], dt)
        if acc_hook is not None:
            acc = acc_hook(acc, z)
        v = c.alpha * acc
        if bias is not None:
            v = v + bias.to(dt)[None, :]
        if inp["row_bias"] is not None:
            v = v + inp["row_bias"].to(dt)[torch.arange(m) // g["row_div"]]
        if c.geglu:
            v = v[:, :n // 2] * v[:, n // 2:]                # value * gelu(gate), gelu(gate) == gate: see the module docstring
        v = v * c.out_scale
        if inp["residual"] is not None:
            v = v + inp["residual"].to(dt)[z * m:(z + 1) * m]
        out.append(v)
    return torch.cat(out)


def gate_preactivation(c, inp):
    """GEGLU: the gate half before the GELU (must be an integer in [8, 255]; 8 everywhere in pass (b))"""
    g = geometry(c)
    return _acc(c, g, inp["a"], inp["w"], torch.float64)[:, c.n // 2:] + inp["bias"][None, c.n // 2:]


def unit(c):
    """what every epilogue term of an output is an integer multiple of: 1, or 8 in GEGLU pass (b) (8 * (sum + integer bias))"""
    return 8.0 if c.geglu == "b" else 1.0


def quantum(c, rows, cols):
    """d: the smallest change of an output that one dropped or doubled product causes; scalar, or [rows, cols] on MXFP8 cases"""
    d = abs(c.alpha * c.out_scale) * (8.0 if c.geglu == "b" else 1.0)
    if c.mx and c.mx_rc:
        g = geometry(c)
        _, _, gr, hc = mx_exponents(c, rows, c.n, g["kc"], g["k"], output=True)
        return d * torch.exp2((gr[:, None] + hc[None, :cols]).double())
    return d


def store(c, v):
    """the ONE rounding"""
    return v.float() if c.out_f32 else v.float().to(BF16)


def differences(c, got, want, tile=None, limit=6):
    """None when got == want (signed zero is one value), else the report a failing kernel is debugged from: how many outputs,
    the first few (row, col, got, want), and the residues of the differing rows / columns modulo 16, 64 and the tile."""
    g, w = got.float(), want.float()
    if g.shape == w.shape and torch.equal(g, w):
        return None
    if g.shape != w.shape:
        return f"{c.name} [{c.target}]: shape {tuple(g.shape)} != {tuple(w.shape)}"
    bad = (g != w) | torch.isnan(g)
    idx = bad.nonzero()
    rows, cols = idx[:, 0], idx[:, 1]
    first = ", ".join(f"({int(r)}, {int(q)}, {float(g[r, q])!r}, {float(w[r, q])!r})" for r, q in idx[:limit].tolist())
    tm, tn = tile or tile_of(c.target)
    res = "; ".join(f"rows mod {mod}: {sorted(set((rows % mod).tolist()))[:16]}" for mod in (16, 64, tm))
    res += "; " + "; ".join(f"cols mod {mod}: {sorted(set((cols % mod).tolist()))[:16]}" for mod in (16, 64, tn))
    return (f"{c.name} [{c.target}]: {int(bad.sum())} of {g.numel()} outputs differ; first (row, col, got, want): {first}; "
            f"{res}; row range {int(rows.min())}..{int(rows.max())}, col range {int(cols.min())}..{int(cols.max())}")


def tile_of(target):
    """(rows, columns) of the output tile of a kernel instance"""
    import re
    t = [x.strip() for x in re.search(r"<(.*)>", target).group(1).split(",")] if "<" in target else []
    if target.startswith("gemm_kernel") or target.startswith("gemm_mx_kernel"):
        return 64 * int(t[1]), 64 * int(t[2])
    if target.startswith("gemm_wide_kernel"):
        return 256, 64 * int(t[1])
    if target.startswith("gemm16_kernel"):
        return 80 * int(t[5]), 160
    if target.startswith("conv_halo_kernel"):
        return 80 * int(t[1]), 160
    if target.startswith("gemm_ws_kernel"):
        return 64, 256 if t[0] == "4" else 320
    return 256, 256                                            # gemm8_kernel


# ------------------------------------------------------------------------------------------------------------- the table
def _tf(v):
    return "true" if v else "false"


G = {"lin": 0, "3x3": 1, "s2": 1, "up": 1, "pad0": 1, "t3": 2}
# epilogue flavours dealt over the instances of a family
EPI = [dict(), dict(residual=True), dict(row_bias=True), dict(residual=True, alpha=0.5, out_scale=2.0),
       dict(out_f32=True, row_bias=True, residual=True), dict(alpha=0.5), dict(out_scale=2.0, row_bias=True), dict(bias=False, residual=True)]


def _cases():
    out = []

    def add(name, target, kind, n, **kw):
        out.append(Case(name=name, target=target, kind=kind, n=n, **kw))

    # ---- gemm.hip: gemm_kernel<gather, tm, tn, pipe>, forced with TC_GEMM_TILE (+ TC_GEMM_PIPE=0).  Two tiles and a ragged
    # tail in M and N for every tile size; K-steps of 64: 3 / 4 (linear), 9 / 18 (3x3), 3 / 6 (T3)
    conv_shapes = {(1, 1, True): ("3x3", 2, 7, 9, 64), (1, 1, False): ("s2", 2, 10, 16, 128), (1, 2, True): ("up", 2, 5, 8, 64),
                   (1, 2, False): ("pad0", 2, 10, 16, 64), (2, 1, True): ("3x3", 3, 7, 9, 128), (2, 1, False): ("3x3", 2, 10, 16, 64),
                   (2, 2, True): ("s2", 3, 14, 18, 64), (2, 2, False): ("up", 3, 5, 8, 64)}
    i = 0
    for tm in (1, 2):
        for tn in (1, 2):
            for pipe in (True, False):
                e = {"TC_GEMM_TILE": f"{tm}{tn}"}
                if not pipe:
                    e["TC_GEMM_PIPE"] = "0"
                n = 64 * tn + 8
                tag = f"{tm}{tn}{'p' if pipe else ''}"
                add(f"tile-lin-{tag}", f"gemm_kernel<0, {tm}, {tn}, {_tf(pipe)}>", "lin", n, m=128 * tm + 11, k=192 if pipe else 256,
                    env=e, **EPI[i % 8])
                kind, fr, h, w, cin = conv_shapes[(tm, tn, pipe)]
                add(f"tile-{kind}-{tag}", f"gemm_kernel<1, {tm}, {tn}, {_tf(pipe)}>", kind, n, frames=fr, h=h, w=w, cin=cin, env=e,
                    **EPI[(i + 3) % 8])
                t3 = dict(frames=6, t_len=3, w=21) if tm == 1 else dict(frames=32, t_len=16, w=7)
                add(f"tile-t3-{tag}", f"gemm_kernel<2, {tm}, {tn}, {_tf(pipe)}>", "t3", n, cin=64 if pipe else 128, env=e, **t3,
                    **EPI[(i + 5) % 8])
                i += 1
    t22 = "gemm_kernel<0, 2, 2, true>"
    add("tile-lin-chunked", "gemm_kernel<0, 1, 1, true>", "lin", 1032, m=139, k=192, ldw=2176, residual=True,
        env={"TC_GEMM_TILE": "11", "TC_GEMM_NMAJOR": "0", "TC_GEMM_ORDER_MIB": "1"}, args=" 1 8 0")
    add("tile-lin-nmajor", t22, "lin", 264, m=267, k=192, row_bias=True, env={"TC_GEMM_TILE": "22", "TC_GEMM_NMAJOR": "2"}, args=" 1 -1 0")
    add("tile-3x3-nmajor", "gemm_kernel<1, 1, 1, true>", "3x3", 136, frames=2, h=7, w=9, cin=64, residual=True,
        env={"TC_GEMM_TILE": "11", "TC_GEMM_NMAJOR": "2"}, args=" 1 -1 0")
    add("tile-lin-epilate", t22, "lin", 136, m=267, k=256, row_bias=True, residual=True, alpha=0.5, out_scale=2.0,
        env={"TC_GEMM_TILE": "22", "TC_GEMM_EPI_LATE": "1"}, args=" 1 0 1")
    add("tile-t3-epilate", "gemm_kernel<2, 1, 2, true>", "t3", 136, frames=6, t_len=3, w=21, cin=64, residual=True,
        env={"TC_GEMM_TILE": "12", "TC_GEMM_EPI_LATE": "1"}, args=" 1 -1 1")         # few rows, big W: the W-stationary walk
    red = ("splitk_reduce_kernel",)
    add("tile-lin-splitk2", t22, "lin", 136, m=267, k=1088, residual=True, env={"TC_GEMM_SPLITK": "2"}, args=" 2 0 0", also=red)
    add("tile-lin-splitk4-k2560", t22, "lin", 136, m=267, k=2560, row_bias=True, env={"TC_GEMM_SPLITK": "4"}, args=" 4 0 0", also=red)
    add("tile-3x3-splitk2", "gemm_kernel<1, 2, 2, true>", "3x3", 136, frames=3, h=7, w=9, cin=128, residual=True,
        env={"TC_GEMM_SPLITK": "2"}, args=" 2 -1 0", also=red)
    add("tile-t3-splitk2", "gemm_kernel<2, 2, 2, true>", "t3", 136, frames=6, t_len=3, w=63, cin=384, out_f32=True,
        env={"TC_GEMM_SPLITK": "2"}, args=" 2 -1 0", also=red)
    add("tile-lin-batch2", t22, "lin", 136, m=267, k=192, batch=2, residual=True, env={"TC_GEMM_TILE": "22"})
    for ps in "ab":
        add(f"tile-geglu-22-{ps}", t22, "lin", 256, m=267, k=320, geglu=ps, env={"TC_GEMM_TILE": "22"})
        add(f"tile-geglu-12-{ps}", "gemm_kernel<0, 1, 2, false>", "lin", 256, m=139, k=256, geglu=ps,
            env={"TC_GEMM_TILE": "12", "TC_GEMM_PIPE": "0"})
    add("tile-geglu-22-rounding", t22, "lin", 256, m=267, k=192, geglu="a", rounding=True, env={"TC_GEMM_TILE": "22"})
    add("tile-lin-rounding", t22, "lin", 136, m=267, k=192, rounding=True, residual=True, env={"TC_GEMM_TILE": "22"})
    add("tile-lin-strided", t22, "lin", 136, m=267, k=192, strided=True, residual=True, env={"TC_GEMM_TILE": "22"})
    add("tile-lin-mirrored", t22, "lin", 136, m=267, k=256, mirrored=True, env={"TC_GEMM_TILE": "22"})
    add("tile-3x3-mirrored", "gemm_kernel<1, 2, 2, true>", "3x3", 136, frames=2, h=10, w=16, cin=64, mirrored=True, env={"TC_GEMM_TILE": "22"})
    add("tile-t3-mirrored", "gemm_kernel<2, 2, 2, true>", "t3", 136, frames=32, w=7, cin=64, mirrored=True, env={"TC_GEMM_TILE": "22"})
    add("tile-lin-n4", "gemm_kernel<0, 1, 1, true>", "lin", 4, m=139, k=192, out_f32=True)          # the scalar epilogue (n % 8 != 0)

    # ---- gemm_wide.hip: gemm_wide_kernel<gather, tnw, pipe>, 256 x (64 tnw) tiles, TC_GEMM_TILE=w (+ TC_GEMM_PIPE=2)
    wide_n = {2: 160, 4: 416, 5: 640}
    wide_conv = {(2, False): ("3x3", 3, 10, 16, 64), (2, True): ("s2", 5, 14, 18, 64), (4, False): ("up", 2, 5, 8, 128),
                 (4, True): ("3x3", 2, 10, 16, 64), (5, False): ("pad0", 5, 14, 18, 64), (5, True): ("3x3", 3, 10, 16, 128)}
    i = 0
    for tnw in (2, 4, 5):
        for pipe in (False, True):
            e = {"TC_GEMM_TILE": "w"}
            if pipe:
                e["TC_GEMM_PIPE"] = "2"
            tag = f"{tnw}{'p' if pipe else ''}"
            add(f"wide-lin-{tag}", f"gemm_wide_kernel<0, {tnw}, {_tf(pipe)}>", "lin", wide_n[tnw], m=300, k=256 if pipe else 192, env=e,
                **EPI[(i + 1) % 8])
            kind, fr, h, w, cin = wide_conv[(tnw, pipe)]
            add(f"wide-{kind}-{tag}", f"gemm_wide_kernel<1, {tnw}, {_tf(pipe)}>", kind, wide_n[tnw], frames=fr, h=h, w=w, cin=cin, env=e,
                **EPI[(i + 4) % 8])
            t3 = dict(frames=32, t_len=16, w=10) if pipe else dict(frames=6, t_len=3, w=63)
            add(f"wide-t3-{tag}", f"gemm_wide_kernel<2, {tnw}, {_tf(pipe)}>", "t3", wide_n[tnw], cin=128 if pipe else 64, env=e, **t3,
                **EPI[(i + 6) % 8])
            i += 1
    w5 = "gemm_wide_kernel<0, 5, false>"
    add("wide-lin-chunked", w5, "lin", 5120, m=300, k=448, env={"TC_GEMM_TILE": "w", "TC_GEMM_ORDER_MIB": "1"}, args=" 8")
    add("wide-lin-batch2", w5, "lin", 640, m=300, k=192, batch=2, residual=True, env={"TC_GEMM_TILE": "w"})
    for ps in "ab":
        add(f"wide-geglu-{ps}", "gemm_wide_kernel<0, 4, false>", "lin", 512, m=300, k=256, geglu=ps, env={"TC_GEMM_TILE": "w"})
    add("wide-lin-rounding", w5, "lin", 640, m=300, k=192, rounding=True, row_bias=True, env={"TC_GEMM_TILE": "w"})
    add("wide-lin-strided", w5, "lin", 640, m=300, k=192, strided=True, residual=True, env={"TC_GEMM_TILE": "w"})
    add("wide-3x3-mirrored", "gemm_wide_kernel<1, 5, false>", "3x3", 640, frames=2, h=10, w=16, cin=64, mirrored=True, env={"TC_GEMM_TILE": "w"})

    # ---- gemm16.hip: gemm16_kernel<gather, pipe, stats, 0, ilv, wm>, 160 x 160 tiles (wm 4: 320 x 160), TC_GEMM_TILE16=2
    g16 = {"false, false, 0, 0, 2": {"TC_G16_ILV": "0"}, "true, false, 0, 0, 2": {"TC_G16_ILV": "0", "TC_GEMM_PIPE": "2"},
           "false, true, 0, 0, 2": {}, "false, false, 0, 1, 2": {"TC_G16_ILV": "1"}, "false, false, 0, 2, 2": {"TC_G16_ILV": "2"},
           "false, false, 0, 0, 4": {"TC_G16_ILV": "0", "TC_G16_TALL": "2"}, "false, false, 0, 1, 4": {"TC_G16_ILV": "1", "TC_G16_TALL": "2"},
           "false, false, 0, 2, 4": {"TC_G16_ILV": "2", "TC_G16_TALL": "2"}}
    g16_conv = ["s2", "up", "3x3", "3x3", "3x3", "pad0", "3x3", "3x3"]           # the request loops 1 / 2 run the plain 3x3 only
    for i, (v, sw) in enumerate(g16.items()):
        e = dict({"TC_GEMM_TILE16": "2"}, **sw)
        stats = v.startswith("false, true")
        tall = v.endswith("4")
        epi = dict(gn_stats=True, residual=True) if stats else EPI[(i + 2) % 8]
        tag = v.replace(", ", "").replace("false", "f").replace("true", "t")
        add(f"g16-lin-{tag}", f"gemm16_kernel<0, {v}>", "lin", 320, m=340, k=192 if i % 2 else 256, env=e, **epi)
        kind = g16_conv[i]
        shape = {"3x3": (3, 10, 16) if tall else (3, 7, 9), "s2": (3, 14, 18), "up": (2, 5, 8), "pad0": (6, 14, 18)}[kind]
        epi = dict(gn_stats=True) if stats else EPI[(i + 5) % 8]
        add(f"g16-{kind}-{tag}", f"gemm16_kernel<1, {v}>", kind, 320, frames=shape[0], h=shape[1], w=shape[2], cin=64 if i % 2 else 128,
            env=e, **epi)
        t3 = dict(frames=6, t_len=3, w=63) if (tall or i % 2) else dict(frames=32, t_len=16, w=7)
        epi = dict(gn_stats=True, row_bias=True) if stats else EPI[(i + 7) % 8]
        add(f"g16-t3-{tag}", f"gemm16_kernel<2, {v}>", "t3", 320, cin=128 if i % 2 else 64, env=e, **t3, **epi)
    g16p = "gemm16_kernel<0, false, false, 0, 0, 2>"
    e16 = {"TC_GEMM_TILE16": "2", "TC_G16_ILV": "0"}
    add("g16-lin-chunked", g16p, "lin", 2560, m=340, k=832, p=1 / 3, env=dict(e16, TC_GEMM_ORDER_MIB="1"), args=" 8")
    add("g16-lin-batch2", g16p, "lin", 320, m=340, k=192, batch=2, residual=True, env=e16)
    add("g16-lin-rounding", g16p, "lin", 320, m=340, k=192, rounding=True, residual=True, env=e16)
    add("g16-lin-strided", g16p, "lin", 320, m=340, k=192, strided=True, residual=True, env=e16)
    add("g16-3x3-mirrored", "gemm16_kernel<1, false, false, 0, 2, 2>", "3x3", 320, frames=3, h=7, w=9, cin=64, mirrored=True,
        env={"TC_GEMM_TILE16": "2", "TC_G16_ILV": "2"})

    # ---- conv_halo.hip: conv_halo_kernel<gather, wm, ks>, 10 x 16 pixel (T3: 16 frames x 10 pixel) patches, TC_CONV_HALO=2
    # (strict: a problem it cannot take FAILS); tall patches with _TALL=2, the K-split form with _KSPLIT=2
    h2 = {"TC_CONV_HALO": "2", "TC_CONV_HALO_KSPLIT": "0"}
    ht = {"TC_CONV_HALO": "2", "TC_CONV_HALO_TALL": "2"}
    hk = {"TC_CONV_HALO": "2", "TC_CONV_HALO_KSPLIT": "2"}
    add("halo-3x3", "conv_halo_kernel<1, 2, 1>", "3x3", 320, frames=2, h=10, w=16, cin=128, env=h2, row_bias=True, residual=True)
    add("halo-3x3-odd", "conv_halo_kernel<1, 2, 1>", "3x3", 320, frames=3, h=10, w=32, cin=64, env=h2, alpha=0.5, out_scale=2.0, residual=True)
    add("halo-3x3-tall", "conv_halo_kernel<1, 4, 1>", "3x3", 320, frames=3, h=20, w=16, cin=64, env=ht, residual=True)
    add("halo-3x3-ksplit", "conv_halo_kernel<1, 2, 2>", "3x3", 320, frames=2, h=10, w=16, cin=256, p=1 / 3, env=hk, row_bias=True)
    add("halo-t3", "conv_halo_kernel<2, 2, 1>", "t3", 320, frames=32, w=10, cin=64, env=h2, residual=True)
    add("halo-t3-even", "conv_halo_kernel<2, 2, 1>", "t3", 320, frames=16, w=30, cin=128, env=h2, out_f32=True, row_bias=True)
    add("halo-t3-tall", "conv_halo_kernel<2, 4, 1>", "t3", 320, frames=32, w=20, cin=128, env=ht, row_bias=True, residual=True)
    add("halo-t3-ksplit", "conv_halo_kernel<2, 2, 2>", "t3", 320, frames=32, w=10, cin=256, env=hk, out_scale=2.0)
    add("halo-3x3-chunked", "conv_halo_kernel<1, 2, 1>", "3x3", 2560, frames=2, h=10, w=16, cin=128, env=dict(h2, TC_GEMM_ORDER_MIB="1"), args=" 8")
    add("halo-3x3-batch2", "conv_halo_kernel<1, 2, 1>", "3x3", 320, frames=2, h=10, w=16, cin=64, batch=2, residual=True, env=h2)
    add("halo-t3-batch2", "conv_halo_kernel<2, 2, 1>", "t3", 320, frames=16, w=20, cin=64, batch=2, env=h2)
    add("halo-3x3-rounding", "conv_halo_kernel<1, 2, 1>", "3x3", 320, frames=2, h=10, w=16, cin=64, rounding=True, residual=True, env=h2)
    add("halo-3x3-strided", "conv_halo_kernel<1, 2, 1>", "3x3", 320, frames=2, h=10, w=16, cin=64, strided=True, residual=True, env=h2)
    add("halo-t3-mirrored", "conv_halo_kernel<2, 2, 1>", "t3", 320, frames=32, w=10, cin=64, mirrored=True, env=h2)

    # ---- gemm_ws.hip: gemm_ws_kernel<4 | 5, geglu, residual, false>, K = 320 only (5 K-steps), 64-row tiles, N slabs of
    # 320 (GEGLU: 256); TC_GEMM_WS = 2 (counted waits) | 3 (vmcnt(0)) | 4 (deeper store window)
    for mode in (2, 3, 4):
        e = {"TC_GEMM_WS": str(mode)}
        safe = {2: 0, 3: 1, 4: 2}[mode]
        add(f"ws-plain-{mode}", "gemm_ws_kernel<5, false, false, false>", "lin", 640, m=200, k=320, env=e, args=f" 4 {safe}")
        add(f"ws-res-{mode}", "gemm_ws_kernel<5, false, true, false>", "lin", 640, m=200, k=320, residual=True, env=e, args=f" 4 {safe}")
        for ps in "ab":
            add(f"ws-geglu-{mode}-{ps}", "gemm_ws_kernel<4, true, false, false>", "lin", 512, m=200, k=320, geglu=ps, env=e, args=f" 4 {safe}")
    add("ws-rounding", "gemm_ws_kernel<5, false, true, false>", "lin", 640, m=200, k=320, rounding=True, residual=True, env={"TC_GEMM_WS": "2"})
    add("ws-strided", "gemm_ws_kernel<5, false, true, false>", "lin", 640, m=200, k=320, strided=True, residual=True, env={"TC_GEMM_WS": "2"})
    add("ws-mirrored", "gemm_ws_kernel<5, false, false, false>", "lin", 640, m=200, k=320, mirrored=True, env={"TC_GEMM_WS": "4"})

    # ---- gemm8.hip: gemm8_kernel<gather, 0>, 256 x 256 tiles walked by persistent blocks, TC_GEMM8=2.  TC_G8_GRID=8: 12 tiles
    # on 8 blocks, so four blocks walk two tiles and four end after one (no next tile to prefetch)
    e8 = {"TC_GEMM8": "2"}
    e88 = {"TC_GEMM8": "2", "TC_G8_GRID": "8"}
    add("g8-lin", "gemm8_kernel<0, 0>", "lin", 264, m=300, k=192, env=e8, residual=True, args=" 4 0")
    add("g8-lin-even", "gemm8_kernel<0, 0>", "lin", 264, m=300, k=128, env=e8, args=" 4 0")             # two K-tiles only
    add("g8-3x3", "gemm8_kernel<1, 0>", "3x3", 264, frames=2, h=10, w=16, cin=64, env=e8, row_bias=True, residual=True)
    add("g8-3x3-even", "gemm8_kernel<1, 0>", "3x3", 264, frames=5, h=7, w=9, cin=128, env=e8)
    add("g8-t3", "gemm8_kernel<2, 0>", "t3", 264, frames=6, t_len=3, w=63, cin=64, env=e8, residual=True)
    add("g8-t3-even", "gemm8_kernel<2, 0>", "t3", 264, frames=32, w=10, cin=128, env=e8, row_bias=True)
    add("g8-lin-grid8", "gemm8_kernel<0, 0>", "lin", 1000, m=700, k=256, env=e88, residual=True, args=" 12 0")
    add("g8-3x3-grid8", "gemm8_kernel<1, 0>", "3x3", 1288, frames=3, h=10, w=16, cin=64, env=e88, args=" 12 0")
    add("g8-t3-grid8", "gemm8_kernel<2, 0>", "t3", 1288, frames=6, t_len=3, w=63, cin=64, env=e88, residual=True, args=" 12 0")
    add("g8-lin-batch2", "gemm8_kernel<0, 0>", "lin", 264, m=300, k=192, batch=2, residual=True, env=e8)
    for ps in "ab":
        add(f"g8-geglu-{ps}", "gemm8_kernel<0, 0>", "lin", 1024, m=300, k=192, geglu=ps, env=e8)
    add("g8-lin-rounding", "gemm8_kernel<0, 0>", "lin", 264, m=300, k=192, rounding=True, residual=True, env=e8)
    add("g8-lin-strided", "gemm8_kernel<0, 0>", "lin", 264, m=300, k=192, strided=True, residual=True, env=e88)
    add("g8-3x3-mirrored", "gemm8_kernel<1, 0>", "3x3", 264, frames=2, h=10, w=16, cin=64, mirrored=True, env=e8)

    # ---- gemm_mx.hip: gemm_mx_kernel<gather, 1, 1> (64 x 64 tiles: fewer than 384 128-tiles and no GEGLU) and <gather, 2, 2>;
    # K-steps of 128 (cin = 192: a K-step straddles two taps).  Operands are 0 or +-2^e per 32-block, which the MX quantiser keeps exactly
    add("mx-lin-11", "gemm_mx_kernel<0, 1, 1>", "lin", 72, m=139, k=384, mx=True, residual=True)
    add("mx-lin-11-even", "gemm_mx_kernel<0, 1, 1>", "lin", 136, m=139, k=512, mx=True, row_bias=True, out_f32=True)
    add("mx-3x3-11", "gemm_mx_kernel<1, 1, 1>", "3x3", 72, frames=2, h=7, w=9, cin=64, mx=True, residual=True)
    add("mx-s2-11", "gemm_mx_kernel<1, 1, 1>", "s2", 72, frames=2, h=10, w=16, cin=128, mx=True)
    add("mx-up-11", "gemm_mx_kernel<1, 1, 1>", "up", 72, frames=2, h=5, w=8, cin=64, mx=True, row_bias=True)
    add("mx-pad0-11", "gemm_mx_kernel<1, 1, 1>", "pad0", 72, frames=2, h=10, w=16, cin=64, mx=True)
    add("mx-t3-11", "gemm_mx_kernel<2, 1, 1>", "t3", 72, frames=6, t_len=3, w=21, cin=128, mx=True, residual=True)
    add("mx-t3-11-t16", "gemm_mx_kernel<2, 1, 1>", "t3", 136, frames=32, w=7, cin=192, mx=True, out_scale=2.0)
    for ps in "ab":
        add(f"mx-geglu-22-{ps}", "gemm_mx_kernel<0, 2, 2>", "lin", 256, m=267, k=384, mx=True, mx_rc=False, geglu=ps)
    add("mx-lin-22", "gemm_mx_kernel<0, 2, 2>", "lin", 2560, m=2450, k=384, mx=True, p=1 / 3, residual=True)
    add("mx-3x3-22", "gemm_mx_kernel<1, 2, 2>", "3x3", 2560, frames=2, h=35, w=35, cin=64, mx=True, p=1 / 3)
    add("mx-t3-22", "gemm_mx_kernel<2, 2, 2>", "t3", 2560, frames=32, w=77, cin=128, mx=True, p=1 / 3, residual=True)
    add("mx-lin-rounding", "gemm_mx_kernel<0, 1, 1>", "lin", 136, m=139, k=384, mx=True, mx_rc=False, rounding=True, residual=True)
    add("mx-lin-strided", "gemm_mx_kernel<0, 1, 1>", "lin", 136, m=139, k=384, mx=True, strided=True, residual=True)
    add("mx-3x3-mirrored", "gemm_mx_kernel<1, 1, 1>", "3x3", 136, frames=2, h=7, w=9, cin=64, mx=True, mirrored=True)
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
