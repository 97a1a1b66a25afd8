#!/usr/bin/env python3
"""usage: lib_ab.py <other libtooncrafter_hip.so> [--new <another build>] [--edges | --fused]
The in-tree library against another BUILD of it (e.g. the previous commit's, kept under scripts/bin/prev/), interleaved in
one process on the UNet's GEMM shapes and fused launches at B = 2 under the default routing; checks that both builds give the same bits.

  --new PATH   take PATH instead of the in-tree library as "new" (the other build in BOTH roles: what two runs of the same
               code differ by -- the noise of the timing columns, the determinism of the battery)
  --fused      time only the fused launches, the temporal and spatial attention, the MXFP8 quantiser and the LayerNorm that
               carries it (the last two sections), not the GEMM / convolution shapes
  --edges      no timing: the same old / new "same bits" check at the smallest shapes where each path of the kernel
               families can go wrong (ragged M, N tails, a ragged last K-step, every epilogue option), the family forced by
               its routing switch, inputs from a seeded CPU generator.  TC_ATTN_STAGE is latched per process: run --edges a
               second time with TC_ATTN_STAGE=reg in the environment for the register-staged attention kernel
"""
import contextlib, ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tooncrafter_amd import _lib, ops
from tooncrafter_amd._lib import ACT_GEGLU, ACT_NONE, ACT_SILU
dev, BF = "cuda", torch.bfloat16
hip = ops.HipOps()       # the ctypes binding: its library handle is swapped per arm (the custom-op layer is linked to the in-tree build)

def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    return lib

args = [a for a in sys.argv[1:] if a not in ("--edges", "--fused")]
edges = "--edges" in sys.argv[1:]
new = hip.lib
if "--new" in args:
    i = args.index("--new"); new = load(args[i + 1]); del args[i:i + 2]
old = load(args[0])
assert old.tc_abi_version() == new.tc_abi_version()

def timeit(fn, iters=20, reps=3):
    fn(); torch.cuda.synchronize(); ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters): fn()
        e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1) / iters)
    return min(ts)

def ab(fn, flops, tag):
    r, outs = {"old": [], "new": []}, {}
    for _ in range(2):
        for name, lib in (("old", old), ("new", new)):
            hip.lib = lib
            outs[name] = fn()
            r[name].append(timeit(fn))
    hip.lib = new
    same = torch.equal(outs["old"], outs["new"])
    a, b = min(r["old"]) * 1e3, min(r["new"]) * 1e3
    spread = (max(r["old"]) - min(r["old"])) / min(r["old"])          # what two timings of the SAME code differ by, this row
    print(f"{tag:40s} old {a:7.1f} us {flops / a / 1e6:7.1f} TF/s | new {b:7.1f} us {flops / b / 1e6:7.1f} TF/s | x{a / b:5.3f} | "
          f"old repeats {100 * spread:4.1f} % apart | {'same bits' if same else 'DIFFERENT BITS'}", flush=True)

def lin(m, n, k, tag, act=ACT_NONE, res=True):
    a = torch.randn(m, k, device=dev).to(BF); w = (torch.randn(n, k, device=dev) * k ** -0.5).to(BF)
    b = torch.randn(n, device=dev); r = torch.randn(m, n, device=dev).to(BF) if res and act != ACT_GEGLU else None
    ab(lambda: hip.gemm(a, w, b, act=act, residual=r), 2.0 * m * n * k, f"linear {tag} {m}x{n}x{k}")

def conv(frames, h, w, cin, cout, tag, t3=False):
    x = torch.randn(frames * h * w, cin, device=dev).to(BF)
    taps = 3 if t3 else 9
    wt = (torch.randn(cout, taps * cin, device=dev) * (taps * cin) ** -0.5).to(BF); b = torch.randn(cout, device=dev)
    res = torch.randn(frames * h * w, cout, device=dev).to(BF)
    geom = dict(kind="t3", frames=frames, t_len=16, cin=cin, h_out=h, w_out=w) if t3 else \
        dict(kind="3x3", frames=frames, cin=cin, h_in=h, w_in=w, h_out=h, w_out=w, stride=1, upsample=False)
    ab(lambda: hip.gemm(x, wt, b, conv=geom, residual=res), 2.0 * frames * h * w * cout * taps * cin,
       f"{'convT3' if t3 else 'conv3x3'} {tag} {cin}->{cout}")

# ---------------------------------------------------------------- --edges
_seed = [0]
def rnd(*shape, scale=1.0, dtype=BF):
    _seed[0] += 1
    g = torch.Generator(device="cpu").manual_seed(_seed[0])
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)

@contextlib.contextmanager
def env(**kv):                      # the library reads its switches per call
    kv = {k: str(v) for k, v in kv.items()}
    was = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    gn_was, hip.gn_part = hip.gn_part, kv.get("TC_GN_PART") == "1"
    try:
        yield " ".join(f"{k}={v}" for k, v in kv.items())
    finally:
        hip.gn_part = gn_was
        for k, v in was.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v

bad, counts = [], {}
def same(fn, tag, want=1):
    """fn() -> tensor or tuple of tensors (None allowed), under both builds; a call the route refuses is refused by both.
    want: tensors the case is about (2 with gn_stats: the output and the sums) -- fewer means the route dropped the part
    under test, and the case is reported as not covered, never as the same bits"""
    outs = {}
    for name, lib in (("old", old), ("new", new)):
        hip.lib = lib
        try:
            o = fn()
            outs[name] = tuple(t for t in (o if isinstance(o, tuple) else (o,)) if t is not None)
        except _lib.TooncrafterHipError as e:
            outs[name] = str(e)
    hip.lib = new
    torch.cuda.synchronize()
    o, n = outs["old"], outs["new"]
    if isinstance(o, str) or isinstance(n, str):
        verdict = f"skipped, the route refuses it ({o})" if o == n else "DIFFERENT BITS (one build refuses the call)"
    elif len(o) == len(n) and len(o) < want:
        verdict = "NOT COVERED: the route emits no statistics for this call"
    else:
        verdict = "same bits" if len(o) == len(n) and all(torch.equal(x, y) for x, y in zip(o, n)) else "DIFFERENT BITS"
        verdict += f" ({len(o)} tensor{'s' if len(o) != 1 else ''})"
    if verdict.startswith("DIFFERENT"): bad.append(tag)
    kind = next(k for k in ("same bits", "skipped", "NOT COVERED", "DIFFERENT BITS") if verdict.startswith(k))
    counts[kind] = counts.get(kind, 0) + 1
    print(f"{tag:118s} {verdict}", flush=True)

def epilogue_sets(m, n, geglu, which):
    """(a) everything at once: bias, row bias with a row_div no tile height is a multiple of, SiLU, alpha, out_scale, residual
    as a column slice (ldr > n) -- a GEGLU launch carries no row bias, residual or second activation;  (b) bias, fp32 output;
    (c) what the 8-wave kernel takes: bias, row bias, sliced residual;  (d) bias alone, bf16 (statistics cases: an fp32 output
    carries none)"""
    n_out = n // 2 if geglu else n
    rb = dict(row_bias=rnd((m + 47) // 48, n, dtype=torch.float32), row_div=48, residual=rnd(m, n_out + 16)[:, 8:8 + n_out])
    sets = {"a": dict(alpha=0.9, out_scale=1.1) if geglu else dict(rb, act=ACT_SILU, alpha=0.9, out_scale=1.1),
            "b": dict(out_f32=True), "c": rb, "d": {}}
    return [(s, sets[s]) for s in which]

def gemm_outs(a, w, b, kw, gn):
    o = hip.gemm(a, w, b, gn_stats=gn, **kw)
    return (o[0], o[1].sums if o[1] is not None else None) if gn else o

def e_lin(sw, m, n, k, geglu=False, gn=False, which="ab"):
    a, w, b = rnd(m, k), rnd(n, k, scale=k ** -0.5), rnd(n, dtype=torch.float32)
    for s, kw in epilogue_sets(m, n, geglu, which):
        if geglu: kw = dict(kw, act=ACT_GEGLU)
        with env(**sw) as tag:
            same(lambda: gemm_outs(a, w, b, kw, gn), want=2 if gn else 1, tag=f"linear{' GEGLU' if geglu else ''}{' +gn_stats' if gn else ''} {m}x{n}x{k} ({s}) {tag}")

def e_conv(sw, frames, h, w_, cin, cout, t3=False):
    m, taps = frames * h * w_, 3 if t3 else 9
    x, wt, b = rnd(m, cin), rnd(cout, taps * cin, scale=(taps * cin) ** -0.5), rnd(cout, dtype=torch.float32)
    geom = dict(kind="t3", frames=frames, t_len=16, cin=cin, h_out=h, w_out=w_) if t3 else \
        dict(kind="3x3", frames=frames, cin=cin, h_in=h, w_in=w_, h_out=h, w_out=w_, stride=1, upsample=False)
    for s, kw in epilogue_sets(m, cout, False, "ab"):
        with env(**sw) as tag:
            same(lambda: hip.gemm(x, wt, b, conv=geom, **kw), f"{'convT3' if t3 else 'conv3x3'} {frames}x{h}x{w_} {cin}->{cout} ({s}) {tag}")

@contextlib.contextmanager
def fp8_linear(min_k=None):         # the fp8 routing of ops.HipOps with its row floor lifted: a LayerNorm's consumer is taken at any M
    was = hip.fp8, hip.fp8_min_m, hip.fp8_min_k                     # min_k: the routing's floor for K lowered too (c = 320 rows)
    hip.fp8, hip.fp8_min_m, hip.fp8_min_k = "linear", 1, was[2] if min_k is None else min_k
    try: yield
    finally: hip.fp8, hip.fp8_min_m, hip.fp8_min_k = was

def e_spatial_and_norms():
    """The spatial attention kernels (under TC_ATTN_STAGE=reg in the environment of the process: the register-staged one),
    the 8-bit attention, the MXFP8 quantiser alone and inside LayerNorm, and every GroupNorm / LayerNorm launch form."""
    stage = os.environ.get("TC_ATTN_STAGE", "dma")
    def kv_rows(batch, lk, div): return ((batch + div - 1) // div) * lk
    # a tail block of queries, ragged key tiles, shared K/V, two query blocks, one query and one key
    for batch, heads, lq, lk, div in ((2, 1, 40, 40, 1), (4, 2, 64, 77, 2), (2, 3, 130, 65, 1), (1, 1, 1, 1, 1)):
        c = 64 * heads
        q, k, v = rnd(batch * lq, c), rnd(kv_rows(batch, lk, div), c), rnd(kv_rows(batch, lk, div), c)
        same(lambda: hip.attention(q, k, v, batch=batch, heads=heads, lq=lq, lk=lk, kv_bdiv=div),
             f"attention b={batch} heads={heads} lq={lq} lk={lk} kv_bdiv={div} stage={stage}")
    qkv = rnd(2 * 100, 3 * 128)                                  # q / k / v as column slices: row stride 3c
    same(lambda: hip.attention(qkv[:, :128], qkv[:, 128:256], qkv[:, 256:], batch=2, heads=2, lq=100, lk=100),
         f"attention b=2 heads=2 lq=100 lk=100 q/k/v slices of [rows, 3c] stage={stage}")
    q, k, v, base = rnd(2 * 96, 128), rnd(2 * 200, 128), rnd(2 * 200, 128), rnd(2 * 96, 128)
    k[150] = q[7] * 4.0                                          # one key far above the rest, late: the rescale runs
    same(lambda: hip.attention(q, k, v, batch=2, heads=2, lq=96, lk=200, out=base.clone(), accumulate=True),
         f"attention b=2 heads=2 lq=96 lk=200 accumulate, spiked key stage={stage}")
    for batch, heads, lq, lk, div, lk2, div2 in ((8, 2, 100, 77, 4, 16, 1), (2, 3, 130, 200, 1, 65, 2), (3, 1, 1, 1, 1, 1, 1)):
        c = 64 * heads
        q, kv, kv2 = rnd(batch * lq, c), rnd(kv_rows(batch, lk, div), 2 * c), rnd(kv_rows(batch, lk2, div2), 2 * c)
        same(lambda: hip.attention(q, kv[:, :c], kv[:, c:], batch=batch, heads=heads, lq=lq, lk=lk, kv_bdiv=div,
                                   k2=kv2[:, :c], v2=kv2[:, c:], lk2=lk2, kv2_bdiv=div2),
             f"attention dual b={batch} heads={heads} lq={lq} lk={lk}/{div} lk2={lk2}/{div2}")
    for batch, heads, lq, lk in ((1, 2, 200, 200), (2, 1, 130, 65)):          # ragged tiles, two query blocks
        c = 64 * heads
        q, k, v = rnd(batch * lq, c), rnd(batch * lk, c), rnd(batch * lk, c)
        same(lambda: hip.attention_q8(q, k, v, batch=batch, heads=heads, lq=lq, lk=lk), f"attention_q8 b={batch} heads={heads} lq={lq} lk={lk}")
    for rows, k, ld in ((64, 32, 64), (5, 96, 96), (33, 2560, 2688)):        # ld > k; scale padding columns (k = 32, 96, 2560: lds = 4, 4, 80)
        x = rnd(rows, ld, scale=3.0)
        same(lambda: hip.quant_mxfp8(x, k), f"quant_mxfp8 rows={rows} k={k} ld={ld}", want=2)
    def ln_mx(x, g, b):
        o = hip.layernorm(x, g, b, mx_for=(4 * x.shape[1], 4 * x.shape[1]))
        return (o.q, o.scales) if isinstance(o, ops.MxRows) else o           # one tensor only: not covered
    # (NV, R) = (2, 2) twice -- 960 pads its scales -- and (4, 1); then (1, 4), c <= 512: a tail group of rows, 320 pads its scales
    for rows, c in ((77, 640), (33, 960), (5, 2048), (9, 320), (130, 512)):
        x, g, b = rnd(rows, c, scale=3.0), rnd(c, scale=0.1, dtype=torch.float32) + 1.0, rnd(c, scale=0.1, dtype=torch.float32)
        with fp8_linear(min_k=320):
            same(lambda: ln_mx(x, g, b), f"layernorm -> MXFP8 {rows}x{c}", want=2)
    for rows, c in ((5, 1280), (333, 512)):
        x, g, b = rnd(rows, c, scale=3.0), rnd(c, scale=0.1, dtype=torch.float32) + 1.0, rnd(c, scale=0.1, dtype=torch.float32)
        same(lambda: hip.layernorm(x, g, b), f"layernorm {rows}x{c}")
    w_pf = rnd(1024, 1024)                                                   # 2 MiB: above the prefetch rule's floor
    # c = 320: a unit is 5 vectors, 51 rows per pass of 256 threads -- 4 vectors a thread up to 204 rows, 13 up to 663; 7000 rows
    # of one sample are 8 slabs and 4.5 MB: the three launches
    for samples, rows, what in ((3, 100, "one pass NV=4"), (2, 500, "one pass NV=13"), (1, 7000, "three launches")):
        x, g, b = rnd(samples * rows, 320, scale=2.0) + 0.5, rnd(320, scale=0.1, dtype=torch.float32) + 1.0, rnd(320, scale=0.1, dtype=torch.float32)
        for silu in (False, True):
            same(lambda: hip.groupnorm(x, g, b, samples=samples, rows=rows, eps=1e-5, silu=silu), f"groupnorm {samples}x{rows}x320 silu={int(silu)} ({what})")
        same(lambda: hip.groupnorm(x, g, b, samples=samples, rows=rows, eps=1e-5, silu=True, prefetch=[w_pf]),
             f"groupnorm {samples}x{rows}x320 silu=1 prefetch 2 MiB ({what})")
    # tc_groupnorm_part: the producer's sums (per block of 160 rows and per channel: sum, sum of squares) stated on the CPU
    samples, rows = 2, 320
    x, g, b = rnd(samples * rows, 320, scale=2.0) + 0.5, rnd(320, scale=0.1, dtype=torch.float32) + 1.0, rnd(320, scale=0.1, dtype=torch.float32)
    xb = x.float().cpu().view(-1, 160, 320)
    part = ops.GnPart(torch.stack([xb.sum(1), (xb * xb).sum(1)], 1).contiguous().to(dev), 160, x)
    for silu in (False, True):
        with env(TC_GN_PART=1) as tag:
            same(lambda: hip.groupnorm(x, g, b, samples=samples, rows=rows, eps=1e-5, silu=silu, part=part), f"groupnorm_part {samples}x{rows}x320 silu={int(silu)} {tag}")

def run_edges():
    for tile in (11, 22):
        for pipe in (0, 1):
            sw = dict(TC_GEMM_TILE=tile, TC_GEMM_PIPE=pipe)
            e_lin(sw, 200, 136, 200)                 # ragged M, N tail inside a tile, 4 K-steps with a ragged last
            e_lin(sw, 200, 12, 200)                  # the scalar tail path
            e_lin(sw, 200, 256, 200, geglu=True)
    # GroupNorm sums of the 128 x 128 tile: a forced tile never emits them (tuning runs only: gemm_route.cpp), so the route is left
    # to itself at the smallest kind of shape it sends there WITH statistics -- at least 384 tiles, n no multiple of 160;
    # ragged M, an N tail, a ragged last K-step
    for pipe in (0, 1): e_lin(dict(TC_GN_PART=1, TC_GEMM_PIPE=pipe), 6200, 1032, 200, gn=True, which="abd")
    e_lin(dict(TC_GEMM_SPLITK=2), 64, 64, 1024)
    for pipe in (1, 2):
        sw = dict(TC_GEMM_TILE="wide", TC_GEMM_PIPE=pipe)
        for n in (160, 256, 320): e_lin(sw, 300, n, 200)
        e_lin(sw, 300, 256, 200, geglu=True)
    for pipe in (1, 2):
        for tall in (0, 2):
            sw = dict(TC_GEMM_TILE16=2, TC_GEMM_PIPE=pipe, TC_G16_TALL=tall)
            e_lin(sw, 200, 320, 200)
            e_lin(dict(sw, TC_GN_PART=1), 200, 320, 200, gn=True, which="abd")
    for ks in (0, 2):
        for tall in (0, 2):
            sw = dict(TC_CONV_HALO=2, TC_CONV_HALO_KSPLIT=ks, TC_CONV_HALO_TALL=tall)
            e_conv(sw, 1, 20 if tall else 10, 16, 256 if ks else 64, 160)
            e_conv(sw, 16, 2, 5, 256 if ks else 64, 160, t3=True)
    e_lin(dict(TC_GEMM8=2), 300, 264, 200, which="c")           # the 8-wave kernel takes neither (a) nor (b)
    for n in (288, 384):                                         # GEGLU: bias only (288 is no multiple of 128: refused; 384 has an N tail)
        a, w, b = rnd(300, 200), rnd(n, 200, scale=200 ** -0.5), rnd(n, dtype=torch.float32)
        with env(TC_GEMM8=2) as tag:
            same(lambda: hip.gemm(a, w, b, act=ACT_GEGLU), f"linear GEGLU 300x{n}x200 (bias) {tag}")
    for heads in (1, 3):                                         # one and three K-steps; x a column slice, ldx > c
        c = 64 * heads
        x, wq, bq = rnd(16 * 8, c + 64)[:, 32:32 + c], rnd(3 * c, c, scale=1.4 * c ** -0.5), rnd(3 * c, scale=0.2, dtype=torch.float32)
        same(lambda: hip.temporal_qkv_attn(x, wq, bq, b=1, t=16, hw=8, heads=heads), f"temporal_qkv_attn b=1 t=16 hw=8 heads={heads} ldx={c + 64}")
    # 17 .. 64 frames (TC_QKV_ATTN=2: every shape reaches the kernel): frames padded to TT = 32 | 64 slots, PX = 128 / TT pixels
    # per tile.  t just above a boundary and at it; hw = PX (one tile per clip) and 12 (three tiles at TT = 32, six at 64);
    # b = 2, so that a tile's padded slots sit against the next clip's rows; one and five K-steps; with and without bias
    def e_tqa(t, hw, heads, bias, pitch=0):
        c = 64 * heads
        x, wq = rnd(2 * t * hw, c + pitch)[:, pitch // 2:pitch // 2 + c], rnd(3 * c, c, scale=1.4 * c ** -0.5)
        bq = rnd(3 * c, scale=0.2, dtype=torch.float32) if bias else None
        with env(TC_QKV_ATTN=2) as tag:
            same(lambda: hip.temporal_qkv_attn(x, wq, bq, b=2, t=t, hw=hw, heads=heads),
                 f"temporal_qkv_attn b=2 t={t} hw={hw} heads={heads} {'bias' if bias else 'no bias'} ldx={c + pitch} {tag}")
    for t in (17, 32, 33, 64):
        for hw in (4 if t <= 32 else 2, 12):
            for heads in (1, 5):
                for bias in (True, False): e_tqa(t, hw, heads, bias)
    e_tqa(33, 12, 5, True, pitch=64)
    # tc_attn_temporal at the same lengths: one wave per (clip, pixel, head), four to a block -- 14 and 70 waves: a tail wave
    for t in (17, 32, 33, 64):
        for heads in (1, 5):
            qkv = rnd(2 * t * 7, 3 * 64 * heads)
            same(lambda: hip.attention_temporal(qkv, b=2, t=t, hw=7, heads=heads), f"attention_temporal b=2 t={t} hw=7 heads={heads}")
    # tc_attn_temporal_rel, every instance (TT = 32 | 64, tables or none) on the same 14 and 70 waves; t = 1 and 5 as well, its
    # domain starts at one frame.  Tables with L = 4 (the distance clamps at every t > 5) and L = 16, without and with the
    # causal mask, and the mask alone
    for t in (1, 5, 16, 17, 32, 33, 64):
        for heads in (1, 5):
            qkv = rnd(2 * t * 7, 3 * 64 * heads)
            for L in (4, 16):
                rk, rv = rnd(2 * L + 1, 64, scale=0.5), rnd(2 * L + 1, 64, scale=0.5)
                for causal in (0, 1):
                    same(lambda: hip.attention_temporal_rel(qkv, rk, rv, b=2, t=t, hw=7, heads=heads, max_rel=L, causal=causal),
                         f"attention_temporal_rel b=2 t={t} hw=7 heads={heads} L={L} causal={causal}")
            same(lambda: hip.attention_temporal_rel(qkv, None, None, b=2, t=t, hw=7, heads=heads, max_rel=0, causal=1),
                 f"attention_temporal_rel b=2 t={t} hw=7 heads={heads} no tables causal=1")
    # the level-0 fused kernels (csrc/fused_l0.h is their shared skeleton; both read their switches per call)
    c = 320
    wq, bq = rnd(3 * c, c, scale=1.4 * c ** -0.5), rnd(3 * c, scale=0.2, dtype=torch.float32)
    wo, bo = rnd(c, c, scale=c ** -0.5), rnd(c, scale=0.2, dtype=torch.float32)
    def e_tb(b, hw, ln_eps=1e-5, pitch=c, **sw):
        x = rnd(b * 16 * hw, pitch)[:, :c]
        with env(TC_TB_FUSED=1, **sw) as tag:
            same(lambda: hip.temporal_attn_fused(x, wq, bq, wo, bo, b=b, t=16, hw=hw, heads=5, ln_eps=ln_eps),
                 f"temporal_attn_fused b={b} t=16 hw={hw} c=320 ldx={pitch} ln_eps={ln_eps} {tag}")
    e_tb(1, 8)                                                   # one tile
    e_tb(1, 24, TC_TB_GRID=1)                                    # three tiles in one block: the stream crosses tile seams
    e_tb(3, 40, TC_TB_GRID=4)                                    # 15 tiles of three clips on 4 blocks: 4, 4, 4 and 3 rounds
    e_tb(1, 8, ln_eps=None)
    e_tb(1, 8, pitch=960)
    e_tb(3, 40, TC_TB_STAGGER=1)
    w1, b1 = rnd(2 * 1280, c, scale=c ** -0.5), rnd(2 * 1280, scale=0.2, dtype=torch.float32)
    w2, b2 = rnd(c, 1280, scale=1280 ** -0.5), rnd(c, scale=0.2, dtype=torch.float32)
    def e_ff(m, ln_eps=1e-5, pitch=c, **sw):
        x = rnd(m, pitch)[:, :c]
        with env(**sw) as tag:
            same(lambda: hip.ff_geglu_fused(x, w1, b1, w2, b2, ln_eps=ln_eps), f"ff_geglu_fused m={m} c=320 hidden=1280 ldx={pitch} ln_eps={ln_eps} {tag}")
    e_ff(100)                                                    # fewer rows than a tile
    e_ff(677, TC_FF_GRID=2)                                      # 6 tiles, 3 per block: tile seams in the stream, a ragged last tile
    e_ff(100, ln_eps=None)
    e_ff(677, pitch=960)
    for sw in (dict(TC_FF_LOOKAHEAD=2), dict(TC_FF_LOOKAHEAD=4), dict(TC_FF_GILP=2)):       # with the default: the four product instances
        e_ff(677, TC_FF_GRID=2, **sw)
    e_spatial_and_norms()
    print("edges: " + ", ".join(f"{v} {k}" for k, v in counts.items()), flush=True)
    print(f"edges: {'no case with different bits' if not bad else f'{len(bad)} DIFFERENT: ' + '; '.join(bad)}", flush=True)
    return 1 if bad else 0

if edges:
    sys.exit(run_edges())
def gemms():
    lin(81920, 960, 320, "L0 qkv", res=False); lin(81920, 640, 320, "L0 640"); lin(20480, 640, 640, "L1 proj"); lin(20480, 1920, 640, "L1 qkv", res=False)
    lin(20480, 640, 2560, "L1 ff2"); lin(5120, 1280, 1280, "L2 proj"); lin(5120, 3840, 1280, "L2 qkv", res=False); lin(5120, 1280, 5120, "L2 ff2")
    lin(5120, 10240, 1280, "L2 geglu", act=ACT_GEGLU); lin(1280, 1280, 1280, "L3 proj"); lin(777, 520, 1288, "ragged")
    conv(32, 10, 16, 1280, 1280, "L2"); conv(32, 10, 16, 2560, 1280, "L2"); conv(32, 5, 8, 1280, 1280, "L3")
    conv(32, 10, 16, 1280, 1280, "L2", t3=True); conv(32, 5, 8, 1280, 1280, "L3", t3=True)
    conv(16, 40, 64, 512, 512, "decoder")
# the fused launches of the temporal / feed-forward blocks at their UNet shapes (B = 2)
def fused():
    c = 320; m = 81920
    x, w1, b1 = rnd(m, c), rnd(2 * 1280, c, scale=c ** -0.5), rnd(2 * 1280, scale=0.2, dtype=torch.float32)
    w2, b2 = rnd(c, 1280, scale=1280 ** -0.5), rnd(c, scale=0.2, dtype=torch.float32)
    ab(lambda: hip.ff_geglu_fused(x, w1, b1, w2, b2, ln_eps=1e-5), 2.0 * m * c * 1280 * 3, f"ff_geglu_fused L0 {m}x{c}x1280")
    wq, bq = rnd(3 * c, c, scale=1.4 * c ** -0.5), rnd(3 * c, scale=0.2, dtype=torch.float32)
    wo, bo = rnd(c, c, scale=c ** -0.5), rnd(c, scale=0.2, dtype=torch.float32)
    with env(TC_TB_FUSED=1):
        ab(lambda: hip.temporal_attn_fused(x, wq, bq, wo, bo, b=2, t=16, hw=2560, heads=5, ln_eps=1e-5), 2.0 * m * c * c * 4, f"temporal_attn_fused L0 {m}x{c}")
    for hw, heads in ((2560, 5), (640, 10), (160, 20)):
        c = 64 * heads; m = 2 * 16 * hw
        x, wq, bq = rnd(m, c), rnd(3 * c, c, scale=1.4 * c ** -0.5), rnd(3 * c, scale=0.2, dtype=torch.float32)
        ab(lambda: hip.temporal_qkv_attn(x, wq, bq, b=2, t=16, hw=hw, heads=heads), 2.0 * m * c * c * 3, f"temporal_qkv_attn {m}x{c}")
    # long clips: the four level geometries of scripts/long_clip_bench.py --qkv-attn at 32 and 64 frames -- the one launch
    # (TC_QKV_ATTN=2: every shape reaches the kernel) and tc_attn_temporal on a qkv tensor of the same geometry
    for hw, heads in ((2560, 5), (640, 10), (160, 20), (40, 20)):
        for t in (32, 64):
            c = 64 * heads; m = 2 * t * hw
            x, wq, bq = rnd(m, c), rnd(3 * c, c, scale=1.4 * c ** -0.5), rnd(3 * c, scale=0.2, dtype=torch.float32)
            with env(TC_QKV_ATTN=2):
                ab(lambda: hip.temporal_qkv_attn(x, wq, bq, b=2, t=t, hw=hw, heads=heads), 2.0 * m * c * c * 3, f"temporal_qkv_attn t={t} {m}x{c}")
            qkv = rnd(m, 3 * c)
            ab(lambda: hip.attention_temporal(qkv, b=2, t=t, hw=hw, heads=heads), 4.0 * m * t * c, f"attention_temporal t={t} {m}x{c}")
    # tc_attn_temporal_rel at level 0 with tables (L = 16) and the causal mask: 16 frames too, it serves every clip length
    rk, rv = rnd(33, 64, scale=0.5), rnd(33, 64, scale=0.5)
    for t in (16, 32, 64):
        m = 2 * t * 2560
        qkv = rnd(m, 3 * 320)
        ab(lambda: hip.attention_temporal_rel(qkv, rk, rv, b=2, t=t, hw=2560, heads=5, max_rel=16, causal=1), 4.0 * m * t * 320,
           f"attention_temporal_rel t={t} {m}x320 L=16 causal")
# the spatial attention kernels, the MXFP8 quantiser and the LayerNorm that carries it, at their UNet shapes (B = 2)
def spatial():
    for batch, heads, l in ((32, 5, 2560), (32, 10, 640)):
        c = 64 * heads
        q, k, v = rnd(batch * l, c), rnd(batch * l, c), rnd(batch * l, c)
        ab(lambda: hip.attention(q, k, v, batch=batch, heads=heads, lq=l, lk=l), 4.0 * batch * heads * l * l * 64, f"attention {batch}x{heads} {l}x{l}")
        if l == 2560:
            ab(lambda: hip.attention_q8(q, k, v, batch=batch, heads=heads, lq=l, lk=l), 4.0 * batch * heads * l * l * 64, f"attention_q8 {batch}x{heads} {l}x{l}")
    q, kv, kv2 = rnd(32 * 2560, 320), rnd(2 * 77, 640), rnd(32 * 16, 640)
    ab(lambda: hip.attention(q, kv[:, :320], kv[:, 320:], batch=32, heads=5, lq=2560, lk=77, kv_bdiv=16, k2=kv2[:, :320], v2=kv2[:, 320:],
                             lk2=16, kv2_bdiv=1), 4.0 * 32 * 5 * 2560 * 93 * 64, "attention dual 32x5 2560x(77/16+16/1)")
    x, g, b = rnd(81920, 320, scale=3.0), rnd(320, scale=0.1, dtype=torch.float32) + 1.0, rnd(320, scale=0.1, dtype=torch.float32)
    ab(lambda: hip.quant_mxfp8(x)[0], 81920.0 * 320, "quant_mxfp8 81920x320")
    with fp8_linear(min_k=320):                                  # k = 320 is below the routing's floor for K: lowered for the row
        ab(lambda: hip.layernorm(x, g, b, mx_for=(1280, 1280)).q, 81920.0 * 320, "layernorm -> MXFP8 81920x320")
if "--fused" not in sys.argv[1:]:
    gemms()
fused()
spatial()
