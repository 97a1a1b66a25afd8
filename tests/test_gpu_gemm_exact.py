"""Every GEMM kernel instance against the bit-exact reference of tests/gemm_exact_cases.py, on the MI355X.

A case runs under its routing switches (tests/test_gemm_exact_cpu.py pins, without a GPU, that they select the instance the
case names) on integer inputs whose correct output is known to the bit: torch.equal, not a tolerance -- every product counted
exactly once, every epilogue operand from the right row and column, one round-to-nearest-even store.  The reference is
float64 torch.matmul / conv2d / conv3d on the CPU and shares no code with tests/emu_ops.py.

A failure names the instance, counts the differing outputs, lists the first few (row, col, got, want) and gives the residues of
the differing rows and columns modulo 16, 64 and the tile: a fragment, a K tail or a tile edge shows in those."""
import pytest
import torch

import gemm_exact_cases as X

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd import _lib
    from tooncrafter_amd.ops import HipOps
    assert (_lib.ACT_NONE, _lib.ACT_GEGLU) == (X.ACT_NONE, X.ACT_GEGLU)
    return HipOps()


@pytest.fixture(scope="module")
def hip_gn():
    """producer statistics ON (tests/test_gpu_gn_part.py): the gemm16 stats instances run only for a call that carries gn_part"""
    from tooncrafter_amd.ops import HipOps
    h = HipOps()
    h.gn_part = True
    return h


@pytest.fixture(scope="module")
def hip8():
    """every eligible GEMM on the MXFP8 route (tests/test_gpu_fp8.py)"""
    from tooncrafter_amd.ops import HipOps
    h = HipOps()
    h.fp8, h.fp8_min_k, h.fp8_min_m, h.fp8_min_n, h.fp8_max_cin, h.fp8_n_over_k = "all", 0, 1, 0, 1 << 20, 0.0
    return h


def _wide(t, cols, at, rows=None):
    """t as the column slice [at, at + t.shape[1]) of a sentinel-filled buffer of `cols` columns (and `rows` rows)"""
    buf = torch.full((rows or t.shape[0], cols), X.SENTINEL, dtype=t.dtype, device=t.device)
    buf[:t.shape[0], at:at + t.shape[1]] = t
    return buf, buf[:t.shape[0], at:at + t.shape[1]]


def launch(h, c, inp):
    """-> (out [batch * m, n_out], the output's whole buffer | None)"""
    from tooncrafter_amd.lvdm.common import pack_geglu
    g = X.geometry(c)
    m, n, k, kc = g["m"], c.n, g["k"], g["kc"]
    n_out = n // 2 if c.geglu else n
    a = inp["a"].to(BF16).to(DEV)
    bias = inp["bias"].float().to(DEV) if inp["bias"] is not None else None
    if c.geglu:
        w, bias = pack_geglu(inp["w"].float().to(DEV), bias)
    else:
        w = inp["w"].to(BF16).to(DEV)
    row_bias = inp["row_bias"].float().to(DEV) if inp["row_bias"] is not None else None
    residual = inp["residual"].to(BF16).to(DEV) if inp["residual"] is not None else None
    odt = torch.float32 if c.out_f32 else BF16
    outbuf = None
    if c.strided:
        _, a = _wide(a, 3 * kc, kc)
        if residual is not None:
            _, residual = _wide(residual, 2 * n_out, n_out)
        outbuf = torch.full((m + 37, 3 * n_out), X.SENTINEL, dtype=odt, device=DEV)
        out = outbuf[:m, n_out:2 * n_out]
    else:
        out = torch.full((c.batch * m, n_out), X.SENTINEL, dtype=odt, device=DEV)
    if c.ldw:
        _, w = _wide(w, c.ldw, 0)
    kw = dict(act=X.ACT_GEGLU if c.geglu else X.ACT_NONE, residual=residual, row_bias=row_bias, row_div=g["row_div"] if c.row_bias else 0,
              alpha=c.alpha, out_scale=c.out_scale, out=out, out_f32=c.out_f32, conv=g["conv"])
    if c.batch > 1:
        kw.update(batch=c.batch, stride_a=g["src_rows"] * kc, stride_w=n * k, stride_c=m * n_out)
        w = w[:n]
    if c.kind == "lin":
        kw["m"] = m
    with X.env(**c.env):
        if c.mx:
            before = dict(h.fp8_calls)
            h.gemm(a, w, bias, **kw)
            assert h.fp8_calls["mx"] == before["mx"] + 1 and h.fp8_calls["bf16"] == before["bf16"], "the fp8 kernel did not run"
        elif c.gn_stats:
            _, part = h.gemm(a, w, bias, gn_stats=True, **kw)
            assert part is not None and part.rows == 160, "the call carried no statistics request: another instance ran"
        else:
            h.gemm(a, w, bias, **kw)
    torch.cuda.synchronize()
    return out, outbuf


@pytest.fixture(scope="module")
def expected():
    """name -> (inputs, stored reference): computed once, on the CPU, never modified"""
    cache = {}

    def get(c):
        if c.name not in cache:
            inp = X.inputs(c)
            cache[c.name] = (inp, X.store(c, X.reference(c, inp)))
        return cache[c.name]
    return get


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_exact(c, expected, request):
    h = request.getfixturevalue("hip8" if c.mx else "hip_gn" if c.gn_stats else "hip")
    inp, want = expected(c)
    out, outbuf = launch(h, c, inp)
    report = X.differences(c, out.cpu(), want)
    assert report is None, report
    if c.strided:
        m, n_out = want.shape
        s = X.SENTINEL
        assert float((outbuf[:m, :n_out].float() - s).abs().max()) == 0 and float((outbuf[:m, 2 * n_out:].float() - s).abs().max()) == 0, \
            f"{c.name} [{c.target}]: columns beside the output slice were written"
        assert float((outbuf[m:].float() - s).abs().max()) == 0, f"{c.name} [{c.target}]: rows behind M were written"
