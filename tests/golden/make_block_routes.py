#!/usr/bin/env python3
"""Generator of tests/golden/block_routes.json: every operator call one BasicTransformerBlock makes -- name, operands,
scalars -- on each route the block can take, and the block's output.

The calls are RECORDED from a tree's own lvdm/attention.py on the emulated operator contract (tests/relpos_cases.py:
RelEmuOps, CPU only, no library): a 64-wide, 1-head block on b = 1, t = 16, h = 2, w = 4 (128 rows);
  * a spatial block (context_dim 96, image cross-attention, 77 + 16 t context tokens) and temporal blocks -- plain,
    relative position, causal, both -- each with every combination of the emulation's offers
    ln_fusion_k (None | 64), ff_fused_c (None | 64), tb_fused_c (None | 64), tqa (False | True): 80 cases;
  * the plain temporal block with tqa on and a `layernorm` that answers `mx_for=` with a non-tensor stand-in (what
    ops.MxRows is on the fp8 route; the recorder's `gemm` unwraps it): 8 cases.  The stand-in may reach `gemm` only.

    python tests/golden/make_block_routes.py [--tree DIR] [--out FILE | --check] [--text FILE]

--tree: the source tree whose tooncrafter_amd is imported (default: this one; the test doubles always come from this
one).  The golden was recorded from the commit BEFORE the block's routing moved into one if-chain per sub-layer, and this
tree reproduces it byte for byte (--check, tests/test_block_routes_cpu.py).  Per case the golden holds the operator
names, the SHA-256 of the full lines and of the output; the lines themselves only for the cases in FULL (--text FILE
writes all of them, to diff two trees when a digest moves).  Parameters and inputs come from integer arithmetic, not from
a random generator, and the emulated operators sum in fp64 (record()), so the digests do not depend on the library
version, the thread count or the CPU's vector units.

Not part of the golden: how often each `*_eligible` rule is asked per sub-layer (`probes` of a case).  The parent asks
ff_fused_eligible twice; this tree asks every rule at most once, which the test asserts."""
import argparse
import hashlib
import itertools
import json
import os
import sys
from functools import partial

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "block_routes.json")
OPS = ("gemm", "attention", "attention_q8", "attention_temporal", "attention_temporal_rel", "temporal_qkv_attn",
       "temporal_attn_fused", "ff_geglu_fused", "layernorm", "groupnorm", "repeat_rows")
RULES = ("gemm_ln_eligible", "ff_fused_eligible", "temporal_attn_fused_eligible", "temporal_qkv_attn_eligible")
B, T, H, W, C = 1, 16, 2, 4, 64
# the cases whose lines the golden keeps in full: nothing offered and everything offered per block kind, and the stand-in axis
FULL = ("spatial plain ln=None ff=None tb=None tqa=False", "spatial plain ln=64 ff=64 tb=64 tqa=True",
        "temporal plain ln=None ff=None tb=None tqa=False", "temporal plain ln=None ff=None tb=None tqa=True",
        "temporal plain ln=64 ff=None tb=None tqa=True", "temporal plain ln=64 ff=64 tb=64 tqa=True",
        "temporal both ln=None ff=None tb=None tqa=True", "temporal both ln=64 ff=64 tb=64 tqa=True",
        "temporal plain ln=None ff=None tb=None tqa=True mx", "temporal plain ln=64 ff=64 tb=None tqa=True mx")


def cases():
    """(name, kind, variant, emulation kwargs, stand-in axis)"""
    offers = list(itertools.product((None, 64), (None, 64), (None, 64), (False, True)))
    out = []
    for kind, variant in (("spatial", "plain"), ("temporal", "plain"), ("temporal", "rel"), ("temporal", "causal"), ("temporal", "both")):
        for ln, ff, tb, tqa in offers:
            out.append((f"{kind} {variant} ln={ln} ff={ff} tb={tb} tqa={tqa}", kind, variant,
                        dict(ln_fusion_k=ln, ff_fused_c=ff, tb_fused_c=tb, tqa=tqa), False))
    for ln, ff, tb, tqa in offers:
        if tqa:
            out.append((f"temporal plain ln={ln} ff={ff} tb={tb} tqa={tqa} mx", "temporal", "plain",
                        dict(ln_fusion_k=ln, ff_fused_c=ff, tb_fused_c=tb, tqa=tqa), True))
    return out


def values(torch, shape, seed, kmax, step):
    """fp32 k * step with integer |k| <= kmax, from a multiplicative hash of the element index (no random generator)."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    h = ((i + 1 + 7919 * seed) * 2654435761) % (1 << 32)
    return (((h >> 13) % (2 * kmax + 1) - kmax).to(torch.float32) * step).reshape(shape)


def recorder_class(torch, rc):
    base = rc.RelEmuOps

    class MxStandIn:
        """What `layernorm(..., mx_for=)` may return instead of a tensor (ops.MxRows): it has a shape and a device, and only
        `gemm` knows what to do with it."""

        def __init__(self, rows):
            self.rows, self.shape, self.device = rows, tuple(rows.shape), rows.device

    class BlockRecorder(base):
        def __init__(self, mx=False, **k):
            super().__init__(**k)
            self.mx, self.depth, self.lines = mx, 0, []
            self.probes, self.sub = {}, {}          # rule -> most probes within one sub-layer; counts of the open sub-layer

        # the two operators that do not go through emu_ops._f, in fp64 like the rest (see record())
        def layernorm(self, x, gamma, beta, eps=1e-5, mx_for=None, prefetch=None):
            y = self._out(torch.nn.functional.layer_norm(x.double(), (x.shape[1],), gamma.double(), beta.double(), eps))
            return MxStandIn(y) if self.mx and mx_for is not None else y

        def attention_temporal_rel(self, qkv, rel_k, rel_v, *, b, t, hw, heads, max_rel, causal, scale=None):
            self.rel_calls += 1
            x = qkv.double().reshape(b, t, hw, 3, heads, 64)
            tabs = [None if r is None else r.double() for r in (rel_k, rel_v)]
            o = rc.rel_attn_f64(x, *tabs, max_rel=max_rel, causal=causal, scale=64 ** -0.5 if scale is None else scale)
            return self._out(o.reshape(b * t * hw, heads * 64)).contiguous()

        def gemm(self, a, w, bias=None, **kw):
            return super().gemm(a.rows if isinstance(a, MxStandIn) else a, w, bias, **kw)

        def describe(self, x):
            if torch.is_tensor(x):
                dig = hashlib.sha256(x.detach().to(torch.float32).contiguous().numpy().tobytes()).hexdigest()[:12]
                return f"{str(x.dtype)[6:]}{list(x.shape)}/{list(x.stride())}#{dig}"
            if isinstance(x, MxStandIn):
                return f"Mx({self.describe(x.rows)})"
            if isinstance(x, (list, tuple)):
                return "[" + ", ".join(self.describe(y) for y in x) + "]"
            return repr(x)

        def __getattribute__(self, name):
            v = object.__getattribute__(self, name)
            if name in RULES:
                def probed(*a, _v=v, _n=name, **kw):
                    self.sub[_n] = self.sub.get(_n, 0) + 1
                    return _v(*a, **kw)
                return probed
            if name in OPS:
                def wrapped(*a, _v=v, _n=name, **kw):
                    if self.depth == 0:              # what the block calls; an emulated fused operator calls others inside
                        if _n == "gemm" and len(a) == 3 and a[2] is None:
                            a = a[:2]                # gemm(a, w, None) is gemm(a, w): one spelling of "no bias"
                        args =[self.describe(x) for x in a] + [f"{k}={self.describe(x)}" for k, x in sorted(kw.items())]
                        self.lines.append(f"{_n}({', '.join(args)})")
                        # a sub-layer ends on the launch that adds its residual
                        if _n in ("temporal_attn_fused", "ff_geglu_fused") or _n == "gemm" and kw.get("residual") is not None:
                            for r, c in self.sub.items():
                                self.probes[r] = max(self.probes.get(r, 0), c)
                            self.sub = {}
                    self.depth += 1
                    try:
                        return _v(*a, **kw)
                    finally:
                        self.depth -= 1
                return wrapped
            return v

    return BlockRecorder


def op_name(line):
    name = line[:line.index("(")]
    return "gemm_ln" if name == "gemm" and "a_norm_eps=" in line and "a_norm_eps=None" not in line else name


def record(tree=ROOT):
    """name -> {"ops", "lines", "out", "probes"} for every case, from the tooncrafter_amd of `tree`"""
    for p in (os.path.join(ROOT, "tests"), tree):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    import torch
    import tooncrafter_amd                           # before the test doubles: tests/conftest.py puts ITS tree first
    from tooncrafter_amd import ops
    from tooncrafter_amd.lvdm.attention import BasicTransformerBlock, ContextCache, CrossAttention
    from tooncrafter_amd.lvdm.common import Act
    import relpos_cases as rc
    assert os.path.realpath(os.path.dirname(os.path.dirname(tooncrafter_amd.__file__))) == os.path.realpath(tree), tooncrafter_amd.__file__
    import emu_ops
    Recorder = recorder_class(torch, rc)
    # The digests must not depend on the machine: the emulated operators sum in fp64 here (their fp32 sums change with
    # the CPU's vector units in the last bit, which now and then moves a bf16 rounding and everything behind it), and the
    # parameters are small multiples of 2^-9, so that folding a LayerNorm into its consumer (fp32, w @ beta) is exact.
    f32, emu_ops._f = emu_ops._f, lambda t: t.to(torch.float64)
    out = {}
    try:
        for name, kind, variant, offers, mx in cases():
            cls = partial(CrossAttention, relative_position=True, temporal_length=T) if variant in ("rel", "both") else None
            blk = BasicTransformerBlock(C, 1, 64, context_dim=96 if kind == "spatial" else None,
                                        image_cross_attention=kind == "spatial", attention_cls=cls).eval()
            with torch.no_grad():
                for i, (pname, p) in enumerate(sorted(blk.named_parameters())):
                    p.copy_(values(torch, p.shape, i, 32, 2.0 ** -9))
                    if pname.startswith("norm") and pname.endswith("weight"):
                        p.add_(1.0)                  # a LayerNorm gain around 1: folding it changes the consumer's weights
            x = values(torch, (B * T * H * W, C), 101, 1024, 2.0 ** -9).to(torch.bfloat16)
            act = Act(x, B, T, H, W)
            rec = Recorder(mx=mx, **offers)
            prev = ops.set_backend(rec)
            try:
                with torch.no_grad():
                    if kind == "spatial":
                        y = blk.forward_spatial(x, act, ContextCache(values(torch, (B, 77 + 16 * T, 96), 102, 1024, 2.0 ** -10), T))
                    else:
                        y = blk.forward_temporal(x, act, causal=variant in ("causal", "both"))
            finally:
                ops.set_backend(prev)
            assert not rec.sub, (name, rec.sub)      # every probe was followed by the launch that closes its sub-layer
            out[name] = {"ops": " ".join(op_name(l) for l in rec.lines), "lines": rec.lines, "out": rec.describe(y),
                         "probes": rec.probes}
    finally:
        emu_ops._f = f32
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def dumps(rec):
    """the golden's text: one case per line, then the full lines of the cases in FULL"""
    def block(items, ind):
        return ",\n".join(ind + x for x in items)
    rows = block([f"{json.dumps(k)}: {json.dumps([v['ops'], digest(v['lines']), v['out']])}" for k, v in rec.items()], "  ")
    full = ",\n".join('  %s: [\n%s\n  ]' % (json.dumps(k), block([json.dumps(l) for l in rec[k]["lines"]], "   ")) for k in FULL)
    return '{\n "shape": %s,\n "cases": {\n%s\n },\n "full": {\n%s\n }\n}\n' % (
        json.dumps({"b": B, "t": T, "h": H, "w": W, "c": C}), rows, full)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with the committed golden instead of writing")
    ap.add_argument("--text", help="also write every line of every case to this file (to diff two trees)")
    a = ap.parse_args()
    rec = record(os.path.abspath(a.tree))
    if a.text:
        with open(a.text, "w") as f:
            f.write("".join(f"[{k}] {l}\n" for k, v in rec.items() for l in v["lines"] + ["-> " + v["out"]]))
    worst = {}
    for v in rec.values():
        for r, c in v["probes"].items():
            worst[r] = max(worst.get(r, 0), c)
    print(len(rec), "cases,", len({v["ops"] for v in rec.values()}), "distinct operator sequences; most probes of a rule "
          "within one sub-layer:", worst)
    g = dumps(rec)
    if a.check:
        same = g == open(GOLDEN).read()
        print("identical to" if same else "DIFFERENT from", GOLDEN)
        return 0 if same else 1
    open(a.out, "w").write(g)
    print("written", a.out, len(g), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
