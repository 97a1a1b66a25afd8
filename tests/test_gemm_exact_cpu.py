"""The table of tests/gemm_exact_cases.py is what it claims, without a GPU:

routing     every bf16 case, as the TcGemmParams line tooncrafter_amd/ops.py would fill, goes through csrc/gemm_route.cpp
            (tests/gemm_route_host_check.cpp, g++) under the case's switches to the instance the case names, with the scalar
            arguments it names; the targets together are the golden's 82 instances minus the three LayerNorm-prologue ones,
            and the six MXFP8 instances;
conditions  from the float64 reference alone: fp32 is exact in any order, every output of a non-rounding case is sensitive
            to one dropped or doubled product, a quarter of a rounding case's outputs are exact ties, the reference equals
            its own float32 re-computation, the MXFP8 operands survive the MX quantiser (oracle/mx.py);
teeth       four seeded defects in the REFERENCE of a long-K linear, a 3x3 convolution and a GEGLU case are each reported by
            the exact comparison -- and the first and the fourth are accepted by check() of tests/test_gpu_ops.py on the
            Gaussian inputs of test_gemm_linear: the gap this suite closes, recorded."""
import importlib.util
import os
import shutil
import subprocess

import pytest
import torch

import gemm_exact_cases as X
from conftest import ROOT
from oracle import mx

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "tooncrafter_amd", "csrc")
BF16 = torch.bfloat16
BY_NAME = {c.name: c for c in X.CASES}


def _gen():
    spec = importlib.util.spec_from_file_location("make_gemm_routes", os.path.join(GOLDEN_DIR, "make_gemm_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def refs():
    """name -> (inputs, V): computed once, never modified"""
    cache = {}

    def get(c):
        if c.name not in cache:
            inp = X.inputs(c)
            cache[c.name] = (inp, X.reference(c, inp))
        return cache[c.name]
    return get


# ------------------------------------------------------------------------------------------------------------- routing
def problem(gen, c):
    """the case as a problem of tests/golden/make_gemm_routes.py: pointers as flags, scratch and statistics 'as ops.py fills them'"""
    g = X.geometry(c)
    n_out = c.n // 2 if c.geglu else c.n
    if c.kind == "lin":
        d = gen.linear(g["m"], c.n, g["k"])
    elif c.kind == "t3":
        d = gen.conv("t3", c.frames, 1, c.w, c.cin, c.n)
        d["t_len"] = c.t_len
    else:
        d = gen.conv(c.kind, c.frames, 2 * c.h if c.kind == "up" else c.h, 2 * c.w if c.kind == "up" else c.w, c.cin, c.n)
    assert (d["m"], d["k"], d["h_out"], d["w_out"]) == (g["m"], g["k"], g["h_out"], g["w_out"]) or c.kind == "lin", (c.name, d)
    d.update(bias=int(c.bias), row_bias=int(c.row_bias), residual=int(c.residual), alpha=c.alpha, out_scale=c.out_scale,
             out_f32=int(c.out_f32), row_div=g["row_div"], act=X.ACT_GEGLU if c.geglu else X.ACT_NONE, ldc=n_out, ldr=n_out,
             gn_part=-1 if c.gn_stats else 0)
    if c.ldw:
        d["ldw"] = c.ldw
    if c.strided:
        d.update(lda=3 * g["kc"], ldc=3 * n_out, ldr=2 * n_out)
    if c.batch > 1:
        d.update(batch=c.batch, stride_a=g["src_rows"] * g["kc"], stride_w=c.n * g["k"], stride_c=g["m"] * n_out)
    return d


@pytest.fixture(scope="module")
def route_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("route") / "gemm_route_host_check"
    r = subprocess.run([gxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                        os.path.join(ROOT, "tests", "gemm_route_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_every_case_routes_to_the_instance_it_names(route_exe):
    gen = _gen()
    by_env = {}
    for c in X.CASES:
        if not c.mx:
            by_env.setdefault(tuple(sorted(c.env.items())), []).append(c)
    for e, cases in by_env.items():
        lines = gen.run(route_exe, dict(e), gen.text([problem(gen, c) for c in cases]))
        assert len(lines) == len(cases)
        for c, line in zip(cases, lines):
            assert line.endswith("| rc=0"), f"{c.name} under {dict(e)}: {line}"
            launches = line.split(" | ")[1:-1]
            assert launches[0].startswith(c.target + " grid="), f"{c.name} under {dict(e)} runs {launches[0]}, not {c.target}"
            assert [l.split(" grid=")[0] for l in launches[1:]] == list(c.also), (c.name, line)
            if c.args:
                assert launches[0].endswith("args=" + c.args), f"{c.name}: scalar arguments {launches[0]!r}, want {c.args!r}"
            if c.gn_stats:
                assert " gn=160 " in line + " ", f"{c.name}: the route offers no statistics: {line}"
    # the chunked walk's threshold (TC_GEMM_ORDER_MIB) is read ONCE per process: a suite that ran any GEMM before keeps the
    # default of 4 MiB, so the chunked cases must reach that walk without the switch as well
    chunked = [c for c in X.CASES if "TC_GEMM_ORDER_MIB" in c.env and not c.mx]
    assert len(chunked) >= 4
    for c in chunked:
        e = {k: v for k, v in c.env.items() if k != "TC_GEMM_ORDER_MIB"}
        (line,) = gen.run(route_exe, e, gen.text([problem(gen, c)]))
        assert line.split(" | ")[1].endswith("args=" + c.args), (c.name, line)


def test_targets_cover_every_instance():
    import json
    with open(os.path.join(GOLDEN_DIR, "gemm_routes.json")) as f:
        kernels = set(json.load(f)["kernels"])
    assert len(kernels) == 82 and X.EXEMPT <= kernels
    bf16 = {c.target for c in X.CASES if not c.mx} | {k for c in X.CASES for k in c.also}
    assert bf16 == kernels - X.EXEMPT, (sorted(kernels - X.EXEMPT - bf16), sorted(bf16 - kernels))
    assert len(bf16) == 79
    assert {c.target for c in X.CASES if c.mx} == X.MX_TARGETS
    for c in X.CASES:
        if c.mx:                      # the tile rule of tc_gemm_mxfp8 (csrc/gemm_mx.hip): 64 x 64 below 384 128-tiles, never for GEGLU
            m = X.geometry(c)["m"]
            small = not c.geglu and ((c.n + 127) // 128) * ((m + 127) // 128) < 384
            assert c.target == f"gemm_mx_kernel<{X.G[c.kind]}, {1 if small else 2}, {1 if small else 2}>", c.name
            assert c.batch == 1 and X.geometry(c)["k"] % 32 == 0 and (c.n // 2 if c.geglu else c.n) % 8 == 0


def test_table_covers_the_scalar_paths_of_every_family():
    """per family: walks, late epilogue, short grid, wait modes, halo forms, split-K, a batch, GEGLU, rounding, strided, mirrored"""
    fam = lambda c: c.target.split("<")[0]
    families = {fam(c) for c in X.CASES}
    assert len(families) == 7
    for f in families:
        mine = [c for c in X.CASES if fam(c) == f]
        assert any(c.rounding for c in mine) and any(c.strided for c in mine) and any(c.mirrored for c in mine), f
        if f not in ("gemm_ws_kernel", "gemm_mx_kernel"):
            assert any(c.batch == 2 for c in mine), f
        if f not in ("conv_halo_kernel", "gemm16_kernel"):
            assert {c.geglu for c in mine} >= {"a", "b"}, f
        if f not in ("gemm_ws_kernel", "gemm8_kernel", "gemm_mx_kernel"):
            assert any("TC_GEMM_ORDER_MIB" in c.env for c in mine), f
        step = 128 if f == "gemm_mx_kernel" else 64
        steps = [(X.geometry(c)["k"] + step - 1) // step for c in mine if c.name != "g8-lin-even"]      # (that one: two K-tiles only)
        assert min(steps) >= 3 and ({s % 2 for s in steps} == {0, 1} or f == "gemm_ws_kernel"), (f, sorted(set(steps)))
    envs = [c.env for c in X.CASES]
    for want in ({"TC_GEMM_NMAJOR": "2"}, {"TC_GEMM_EPI_LATE": "1"}, {"TC_G8_GRID": "8"}, {"TC_GEMM_WS": "2"}, {"TC_GEMM_WS": "3"},
                 {"TC_GEMM_WS": "4"}, {"TC_CONV_HALO_TALL": "2"}, {"TC_CONV_HALO_KSPLIT": "2"}, {"TC_GEMM_SPLITK": "2"}, {"TC_GEMM_SPLITK": "4"}):
        assert any(want.items() <= e.items() for e in envs), want
    for c in X.CASES:
        g = X.geometry(c)
        tm, tn = X.tile_of(c.target)
        assert (g["m"] > tm and c.n > tn) or c.name == "tile-lin-n4", f"{c.name}: fewer than two tiles"
        assert c.batch * g["m"] <= 4096, c.name
        if c.kind != "lin":
            assert c.frames >= 2
    t3 = {c.t_len for c in X.CASES if c.kind == "t3"}
    assert 16 in t3 and len(t3) > 1


# ----------------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_conditions(c, refs):
    inp, v = refs(c)
    g = X.geometry(c)
    n_out = c.n // 2 if c.geglu else c.n
    assert v.shape == (c.batch * g["m"], n_out)
    for key, t in inp.items():                                # A, W and the residual are bf16 values; bias / row_bias are fp32
        if t is not None:
            assert torch.equal(t.to(torch.float32 if "bias" in key else BF16).double(), t)
    # fp32 accumulation is exact in any order
    epi = sum(float(t.abs().max()) for t in (inp["bias"], inp["row_bias"], inp["residual"]) if t is not None)
    quantum_a = float(inp["a"][inp["a"] != 0].abs().min()) * float(inp["w"][inp["w"] != 0].abs().min())
    assert (g["k"] * float(inp["a"].abs().max()) * float(inp["w"].abs().max()) + epi) / min(quantum_a, 1.0) < 2 ** 24
    # the reference is exact: the same operators in float32 give the same numbers
    assert torch.equal(X.reference(c, inp, torch.float32).double(), v), "float64 and float32 references differ"
    if c.geglu:
        gate = X.gate_preactivation(c, inp)
        assert torch.equal(gate, gate.round()) and float(gate.min()) >= 8 and float(gate.max()) <= (1023 if c.rounding else 255)
        if c.geglu == "b":
            assert float(gate.min()) == 8 == float(gate.max()) and float(v.abs().max()) < 2048
    if c.mx:
        for t in (inp["a"], inp["w"]):
            assert torch.equal(mx.fake_quant(t.float()).double(), t), "an operand does not survive the MX quantiser"
        ea, ew, _, _ = X.mx_exponents(c, inp["a"].shape[0], c.n, g["kc"], g["k"])
        assert int(ea.min()) >= -3 and int(ea.max()) <= 3 and int(ew.min()) >= -3 and int(ew.max()) <= 3
        assert len(ea.unique()) >= 4 and len(ew.unique()) >= 4
    if c.rounding:
        stored = X.store(c, v).double()
        ulp = torch.exp2(torch.floor(torch.log2(v.abs())) - 7)          # bf16: 8 significant bits
        ties = (v - stored).abs() * 2 == ulp
        assert float(v.min()) >= 256 and float(v.max()) < 1024
        assert float(ties.double().mean()) >= 0.25, f"only {float(ties.double().mean()):.3f} of the outputs are ties"
        assert bool((stored[ties] > v[ties]).any()) and bool((stored[ties] < v[ties]).any())      # to even: up for some, down for others
    else:
        d = X.quantum(c, v.shape[0], v.shape[1])
        d = d if torch.is_tensor(d) else torch.full_like(v, d)
        u = d.clamp(max=X.unit(c))
        assert torch.equal((v / u).round(), v / u), "an output is no integer multiple of its quantum"
        worst = float(((v.abs() + d) / (256 * u)).max())
        assert worst < 1, f"an output is not sensitive: (|V| + d) / (256 u) = {worst:.3f}"
        assert torch.equal(X.store(c, v).double(), v) and torch.equal(X.store(c, v + d).double(), v + d)


# ---------------------------------------------------------------------------------------------------------------- teeth
def round_half_up(v):
    """bf16 store that rounds ties away from zero instead of to even (fp32 bits + 0x8000, truncated)"""
    bits = v.float().view(torch.int32).to(torch.int64)
    mag = (((bits & 0x7fffffff) + 0x8000) & ~0xffff).to(torch.int32).view(torch.float32)
    return torch.where(bits < 0, -mag, mag).to(BF16)


def _one_product(c, inp, rows, col):
    """a product (+-1 times the case's scales) that EXISTS in the sum of each output (row, col): its value per row"""
    g = X.geometry(c)
    dt = torch.float64
    cnt = torch.cat([X._acc(c, g, inp["a"].abs(), inp["w"].abs(), dt)])[rows, col]
    acc = torch.cat([X._acc(c, g, inp["a"], inp["w"], dt)])[rows, col]
    assert bool((cnt >= 1).all()), "no non-zero product to drop"
    return torch.where(cnt + acc > 0, torch.ones_like(acc), -torch.ones_like(acc))          # a +1 exists unless all are -1


def defect(kind, c, inp):
    """the reference of c with one seeded defect"""
    g = X.geometry(c)
    gen = torch.Generator().manual_seed(X._seed(c, 99))
    m, lo = g["m"], (c.n // 2 if c.geglu == "a" else 0)
    hi = c.n // 2 if c.geglu == "b" else c.n
    col = lo + int(torch.randint(0, hi - lo - 9, (1,), generator=gen))
    row = int(torch.randint(0, m - 16, (1,), generator=gen))
    if kind == "dropped":
        rows = torch.tensor([row])
        val = _one_product(c, inp, rows, col)

        def hook(acc, z):
            acc = acc.clone()
            acc[rows, col] -= val.to(acc.dtype)
            return acc
        return X.reference(c, inp, acc_hook=hook)
    if kind == "doubled":
        rows = torch.arange(row // 16 * 16, row // 16 * 16 + 16)
        val = _one_product(c, inp, rows, col)

        def hook(acc, z):
            acc = acc.clone()
            acc[rows, col] += val.to(acc.dtype)
            return acc
        return X.reference(c, inp, acc_hook=hook)
    if kind == "bias":
        c0 = col // 8 * 8
        bias = inp["bias"].clone()
        bias[c0:c0 + 8] = inp["bias"][c0 + 1:c0 + 9]
        return X.reference(c, inp, bias=bias)
    raise ValueError(kind)


REPRESENTATIVE = {"tile-lin-splitk4-k2560": "tile-lin-rounding", "halo-3x3": "halo-3x3-rounding", "tile-geglu-22-a": "tile-geglu-22-rounding",
                  "tile-geglu-22-b": "tile-geglu-22-rounding"}


@pytest.mark.parametrize("name", list(REPRESENTATIVE))
@pytest.mark.parametrize("kind", ["dropped", "doubled", "bias"])
def test_exact_comparison_reports_a_seeded_defect(name, kind, refs):
    c = BY_NAME[name]
    assert c.batch == 1 and (name != "tile-lin-splitk4-k2560" or c.k == 2560)
    inp, v = refs(c)
    bad = defect(kind, c, inp)
    want = {"dropped": 1, "doubled": 16, "bias": None}[kind]
    report = X.differences(c, X.store(c, bad), X.store(c, v))
    assert report is not None, f"{kind} is invisible"
    assert c.target in report and "rows mod 16" in report and "cols mod 64" in report and "(row, col, got, want)" in report
    n_bad = int((X.store(c, bad).float() != X.store(c, v).float()).sum())
    assert n_bad == want if want else n_bad >= X.geometry(c)["m"], (kind, n_bad)      # the shifted group: every row, up to 8 columns
    assert X.differences(c, X.store(c, v), X.store(c, v)) is None
    assert X.differences(c, -0.0 * X.store(c, v), 0.0 * X.store(c, v)) is None, "signed zero is one value"


@pytest.mark.parametrize("name", sorted(set(REPRESENTATIVE.values())))
def test_exact_comparison_reports_a_round_half_up_store(name, refs):
    """The store's rounding shows only where something is rounded: the non-rounding cases' outputs are bf16 values by
    construction, so this defect is applied to the rounding case of the same family."""
    c = BY_NAME[name]
    _, v = refs(c)
    got, want = round_half_up(v), X.store(c, v)
    assert torch.equal(round_half_up(want.double()), want), "round-half-up must keep a bf16 value"
    assert X.differences(c, got, want) is not None
    assert X.differences(c, (v.float().view(torch.int32) & ~0xffff).view(torch.float32).to(BF16), want) is not None, "truncation is invisible"


def check_accepts(out, ref, rel=4e-3):
    """check() of tests/test_gpu_ops.py, restated (that module imports the library): rel-L2 <= 4e-3, max-abs <= 4 bf16 ulps of scale"""
    o, r = out.double(), ref.double()
    err = float((o - r).norm() / (r.norm() + 1e-30))
    ulps = float((o - r).abs().max()) / ((float(r.abs().max()) + 1e-30) * 2 ** -8)
    return bool(torch.isfinite(o).all()) and err <= rel and ulps <= 4.0


@pytest.mark.parametrize("m,n,k", [(256, 320, 320), (4096, 1280, 2560)])
def test_the_tolerance_check_accepts_what_the_exact_comparison_reports(m, n, k):
    """The gap, recorded: on the Gaussian inputs of test_gemm_linear one product dropped from one output and a
    round-half-up store both pass check()."""
    def rnd(*shape, seed, scale=1.0, dtype=BF16):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(dtype)
    a, w, bias = rnd(m, k, seed=1).float(), rnd(n, k, seed=2, scale=k ** -0.5).float(), rnd(n, seed=3, dtype=torch.float32)
    v = a @ w.t() + bias
    ref = v.to(BF16)
    g = torch.Generator().manual_seed(m + n + k)
    r, q, kk = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (m, n, k))
    dropped = v.clone()
    dropped[r, q] -= a[r, kk] * w[q, kk]
    assert a[r, kk] * w[q, kk] != 0
    assert check_accepts(dropped.to(BF16), ref), "the tolerance check sees a dropped product here: pick the gap elsewhere"
    assert check_accepts(round_half_up(v), ref)
    assert not check_accepts(ref * 1.02, ref)                 # and it is the check it claims to be
