"""The seven kernels of csrc/norm.hip (gn_stats, gn_finalize, gn_finalize_part, gn_apply, gn_onepass<256, 4 | 13>,
layernorm<1,4 | 2,2 | 4,1> and its MXFP8 form, softmax_rows) against the expectations of tests/norm_exact_cases.py, on the
MI355X, through the C ABI (hip.lib.tc_*), so that the caller owns every buffer.

An expectation is float64; the kernels' fp32 arithmetic errs far below half a bf16 ulp, so the comparison is torch.equal where
the expectation is a bf16 value (family A without SiLU, the softmax cases) and |got - ref| <= 1 bf16 ulp of |ref| elementwise
elsewhere (a faithful kernel is within 0.5).  test_norm_exact_cpu.py holds the expectations to their closed forms and to the
seeded defects; nothing here depends on tests/emu_ops.py.  Every output is the leading rows of a sentinel-filled buffer
with PAD_ROWS sentinel rows behind it, and neither those nor the input may change.

A failure names the case and its kernel path, counts the differing outputs, lists the first few (row, channel, got, want,
error in ulps), the (sample, group) pairs or rows they lie in and the residues of their rows and channels."""
import ctypes as C

import pytest
import torch

import norm_exact_cases as X

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
PAD_ROWS = X.PAD_ROWS


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def expected():
    """name -> (inputs, stored expectation) of the one-launch families: computed once, on the CPU, never modified"""
    cache = {}

    def get(c):
        if c.name not in cache:
            inp = X.inputs(c)
            cache[c.name] = (inp, X.expected(c, inp))
        return cache[c.name]
    return get


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(rc, what):
    from tooncrafter_amd import _lib
    _lib.check(rc, what)


def _sentinels(shape, dtype=BF16, value=X.SENTINEL):
    return torch.full(shape, value, dtype=dtype, device=DEV)


class Operands:
    """x, gamma, beta of a case on the device, the output buffer, and a copy of x to hold x to afterwards"""

    def __init__(self, c, inp, front=0):
        self.c, self.front = c, front
        n = c.total_rows
        self.xbuf = _sentinels((front + n + front, c.c))
        self.x = self.xbuf[front:front + n]
        self.x.copy_(inp["x"].to(BF16))
        self.x0 = self.xbuf.clone()
        self.gamma, self.beta = inp["gamma"].float().to(DEV), inp["beta"].float().to(DEV)
        self.buf = _sentinels((front + n + PAD_ROWS, c.c))
        self.y = self.buf[front:front + n]

    def judge(self, want, rule=None, what=""):
        torch.cuda.synchronize()
        c = self.c
        assert torch.equal(self.xbuf, self.x0), f"{what}{c.name} [{c.path}]: the input (or a row beside it) was written"
        assert bool((self.buf[:self.front] == X.SENTINEL).all()), f"{what}{c.name} [{c.path}]: rows in front of the output were written"
        report = X.judge(c, self.buf[self.front:], want, rule, what)
        assert report is None, report


def call_groupnorm(h, o, prefetch=None, part=None, prows=0):
    c = o.c
    nbytes = h.lib.tc_groupnorm_workspace(c.samples, c.rows, c.c)
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)
    head = (o.x.data_ptr(), o.y.data_ptr(), o.gamma.data_ptr(), o.beta.data_ptr())
    tail = (c.samples, c.rows, c.c, float(c.eps), int(c.silu), ws.data_ptr(), nbytes)
    if part is not None:
        _check(h.lib.tc_groupnorm_part(*head, part.data_ptr(), prows, *tail, _stream()), "tc_groupnorm_part")
    elif prefetch is not None:
        _check(h.lib.tc_groupnorm_pf(*head, *tail, C.byref(prefetch), _stream()), "tc_groupnorm_pf")
    else:
        _check(h.lib.tc_groupnorm(*head, *tail, _stream()), "tc_groupnorm")
    torch.cuda.synchronize()                                   # the workspace lives until the launches have run


def call_layernorm(h, o, prefetch=None):
    c = o.c
    args = (o.x.data_ptr(), o.y.data_ptr(), o.gamma.data_ptr(), o.beta.data_ptr(), c.rows, c.c, float(c.eps))
    if prefetch is not None:
        _check(h.lib.tc_layernorm_pf(*args, C.byref(prefetch), _stream()), "tc_layernorm_pf")
    else:
        _check(h.lib.tc_layernorm(*args, _stream()), "tc_layernorm")


def call(h, o, **kw):
    (call_groupnorm if o.c.op == "groupnorm" else call_layernorm)(h, o, **kw)


ONE_LAUNCH = [c for c in X.CASES if c.family != "C"]


@pytest.mark.parametrize("c", [c for c in ONE_LAUNCH if c.op == "groupnorm"], ids=lambda c: c.name)
def test_groupnorm(c, hip, expected):
    inp, want = expected(c)
    o = Operands(c, inp)
    call(hip, o)
    o.judge(want)


@pytest.mark.parametrize("c", [c for c in ONE_LAUNCH if c.op == "layernorm"], ids=lambda c: c.name)
def test_layernorm(c, hip, expected):
    inp, want = expected(c)
    o = Operands(c, inp)
    call(hip, o)
    o.judge(want)                                               # the sentinel rows: a clamped row recomputes, never stores


@pytest.mark.parametrize("c", [c for c in X.CASES if c.family == "C"], ids=lambda c: c.name)
def test_one_spike_per_group(c, hip):
    """family C: the spike walks through every row and channel; inputs and the float64 expectation are built on the device"""
    for launch in range(X.launches(c)):
        inp = X.inputs(c, launch, device=DEV)
        o = Operands(c, inp)
        call(hip, o)
        o.judge(X.expected(c, inp), what=f"launch {launch}: ")


def _first_per_path(cases):
    out = {}
    for c in cases:
        out.setdefault(c.path, c)
    return list(out.values())


# one GroupNorm case per path of the shape table, one LayerNorm case per instance (33 rows: a ragged last block); family B
PER_PATH = _first_per_path(c for c in X.CASES if c.family == "B" and c.seed == 0 and (c.op == "groupnorm" or c.rows == 33))


def test_per_path_holds_every_path():
    assert {c.path for c in PER_PATH} == {p for _, p in X.GN_SHAPES} | {"layernorm<1,4>", "layernorm<2,2>", "layernorm<4,1>"}
    assert len(PER_PATH) == 8


@pytest.mark.parametrize("c", PER_PATH, ids=lambda c: c.name)
def test_neighbours_untouched(c, hip, expected):
    """x and y are the middle rows of sentinel-filled buffers: nothing in front of or behind either may change"""
    inp, want = expected(c)
    o = Operands(c, inp, front=PAD_ROWS)
    call(hip, o)
    o.judge(want)


@pytest.mark.parametrize("c", PER_PATH, ids=lambda c: c.name)
def test_prefetch_planes_change_nothing(c, hip, expected):
    """tc_groupnorm_pf / tc_layernorm_pf with a list of one 1 MiB + 48 byte tensor: the same bits as the plain entry point,
    and the tensor is only read"""
    from tooncrafter_amd.ops import HipOps
    inp, want = expected(c)
    plain = Operands(c, inp)
    call(hip, plain)
    dummy = torch.randint(0, 256, ((1 << 20) + 48,), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    dummy0 = dummy.clone()
    pf = HipOps._prefetch_struct([dummy])
    assert pf.n == 1 and pf.bytes[0] == (1 << 20) + 48
    o = Operands(c, inp)
    call(hip, o, prefetch=pf)
    o.judge(want, what="with prefetch planes: ")
    assert torch.equal(o.buf.view(torch.int16), plain.buf.view(torch.int16)), f"{c.name}: the prefetch planes changed the result"
    assert torch.equal(dummy, dummy0), f"{c.name}: the prefetched tensor was written"


@pytest.mark.parametrize("c,prows", X.PART_CASES, ids=lambda v: v.name if isinstance(v, X.Case) else str(v))
def test_groupnorm_from_hand_made_partial_sums(c, prows, hip):
    """tc_groupnorm_part (gn_finalize_part + gn_apply) on the exact integer sums of a family-B input"""
    inp = X.inputs(c)
    want = X.expected(c, inp)
    part = X.exact_part(inp["x"], prows).to(DEV)
    o = Operands(c, inp)
    call_groupnorm(hip, o, part=part, prows=prows)
    o.judge(want)
    assert torch.equal(part.cpu(), X.exact_part(inp["x"], prows)), "the partial sums were written"


MX_CASES = [X.Case(f"ln-{r}x{w}-{'LB' if fam == 'B' else fam}-mx", "layernorm", fam, 1, r, w, 1e-5, False, 0, "layernorm<MX>")
            for w in X.LN_MX_WIDTHS for r in (5, 33) for fam in ("A", "B")]


@pytest.mark.parametrize("c", MX_CASES, ids=lambda c: c.name)
def test_layernorm_mxfp8_is_the_quantised_layernorm(c, hip):
    """tc_layernorm_mxfp8 == tc_quant_mxfp8(tc_layernorm(x)) byte for byte, the zeroed padding columns of the scales
    included (C = 64 and 320: 2 of them), and nothing behind the two outputs is written"""
    inp = X.inputs(c)
    o = Operands(c, inp)
    call_layernorm(hip, o)
    o.judge(X.expected(c, inp))
    q_want, s_want = hip.quant_mxfp8(o.y.contiguous())
    lds = (c.c + 127) // 128 * 4
    assert s_want.shape[1] == lds and (lds - c.c // 32 == 2) == (c.c in (64, 320))
    q = _sentinels((c.rows + PAD_ROWS, c.c), torch.uint8, 0xA5)
    sc = _sentinels((c.rows + PAD_ROWS, lds), torch.uint8, 0xA5)
    _check(hip.lib.tc_layernorm_mxfp8(o.x.data_ptr(), q.data_ptr(), c.c, sc.data_ptr(), lds, o.gamma.data_ptr(), o.beta.data_ptr(),
                                      c.rows, c.c, float(c.eps), _stream()), "tc_layernorm_mxfp8")
    torch.cuda.synchronize()
    assert torch.equal(o.xbuf, o.x0), f"{c.name}: the input was written"
    nq = int((q[:c.rows] != q_want).sum())
    assert nq == 0, f"{c.name}: {nq} e4m3 bytes differ from the quantised LayerNorm; first at {torch.nonzero(q[:c.rows] != q_want)[:4].tolist()}"
    ns = int((sc[:c.rows] != s_want).sum())
    assert ns == 0, f"{c.name}: {ns} scale bytes differ; first at {torch.nonzero(sc[:c.rows] != s_want)[:4].tolist()}"
    assert bool((sc[:c.rows, c.c // 32:] == 0).all()), f"{c.name}: padding columns of the scales are not zero"
    assert bool((q[c.rows:] == 0xA5).all()) and bool((sc[c.rows:] == 0xA5).all()), f"{c.name}: rows behind the outputs were written"


@pytest.mark.parametrize("c", X.SCASES, ids=lambda c: c.name)
def test_softmax_rows(c, hip):
    """bit for bit: bf16(1 / k) on each row's set, zeros in [n, n_out), sentinels in [n_out, ldo) and in the rows behind"""
    n, n_out, lds, ldo = c.dims
    s = X.s_inputs(c).to(DEV)
    s0 = s.clone()
    buf = _sentinels((c.rows + PAD_ROWS, ldo))
    _check(hip.lib.tc_softmax_rows(s.data_ptr(), buf.data_ptr(), c.rows, n, n_out, lds, ldo, c.causal_period, _stream()), "tc_softmax_rows")
    torch.cuda.synchronize()
    assert torch.equal(s, s0), f"{c.name}: the scores were written"
    report = X.s_judge(c, buf)
    assert report is None, report
