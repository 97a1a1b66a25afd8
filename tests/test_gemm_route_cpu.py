"""Where every bf16 GEMM goes, pinned on the CPU: csrc/gemm_route.cpp is compiled with g++ into
tests/gemm_route_host_check.cpp and run over the problem set of tests/golden/make_gemm_routes.py -- the unique problems
of a full-size forward and decode, the refusal cases, a synthetic grid -- under every switch setting the tests and
scripts use.  tests/golden/gemm_routes.json was RECORDED from the launchers of the commit before the routing moved into
one function (make_gemm_routes.py: hipLaunchKernelGGL turned into a recorder, no GPU), so a routing edit that moves a
layer to another kernel instance, grid or scalar argument shows up here as a changed line."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "tooncrafter_amd", "csrc")
FAMILY_FILES = ["gemm.hip", "gemm16.hip", "gemm8.hip", "gemm_wide.hip", "gemm_ws.hip", "conv_halo.hip", "gemm_common.h"]


def _gen():
    spec = importlib.util.spec_from_file_location("make_gemm_routes", os.path.join(GOLDEN_DIR, "make_gemm_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "gemm_routes.json")) as f:
        return json.load(f)


def test_route_reproduces_the_recorded_launches(tmp_path, golden):
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    gen = _gen()
    exe = tmp_path / "gemm_route_host_check"
    r = subprocess.run([gxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                        os.path.join(ROOT, "tests", "gemm_route_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    dump = open(tmp_path / "lines.txt", "w")
    got = gen.summarise(lambda env, text: gen.run(str(exe), env, text), golden["recorded"], dump)
    dump.close()
    assert got["problems"] == golden["problems"] and list(got["settings"]) == list(golden["settings"])
    for i, (a, b) in enumerate(zip(got["default"], golden["default"])):
        assert a == b, f"recorded / refusal problem {i} under the default setting"
    hint = f"(every line the route gives: {tmp_path / 'lines.txt'}; the launchers': tests/golden/make_gemm_routes.py --text)"
    for name, (real, grid) in golden["settings"].items():
        assert got["settings"][name][0] == real, f"recorded / refusal problems under [{name}] {hint}"
        assert got["settings"][name][1] == grid, f"synthetic grid under [{name}] {hint}"
    assert gen.dumps(got) == open(os.path.join(GOLDEN_DIR, "gemm_routes.json")).read()


def test_golden_covers_every_variant_the_launchers_can_select(golden):
    seen = set(golden["kernels"])
    tf = ("false", "true")
    want = {f"gemm_kernel<{g}, {tm}, {tn}, {p}>" for g in range(3) for tm in (1, 2) for tn in (1, 2) for p in tf}
    want |= {f"gemm_wide_kernel<{g}, {t}, {p}>" for g in range(3) for t in (2, 4, 5) for p in tf}
    want |= {f"gemm16_kernel<{g}, {v}>" for g in range(3) for v in ("false, false, 0, 0, 2", "true, false, 0, 0, 2", "false, true, 0, 0, 2",
                                                                     "false, false, 0, 1, 2", "false, false, 0, 2, 2", "false, false, 0, 0, 4",
                                                                     "false, false, 0, 1, 4", "false, false, 0, 2, 4")}
    want |= {f"conv_halo_kernel<{g}, {v}>" for g in (1, 2) for v in ("2, 1", "4, 1", "2, 2")}
    want |= {f"gemm_ws_kernel<{v}, {ln}>" for v in ("4, true, false", "5, false, true", "5, false, false") for ln in tf}
    want |= {f"gemm8_kernel<{g}, 0>" for g in range(3)} | {"splitk_reduce_kernel"}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    assert len(golden["recorded"]["unet"]) >= 60 and len(golden["recorded"]["decode"]) >= 10


def test_launchers_only_launch():
    """The family files read no routing switch and carry no dry run: the decision is csrc/gemm_route.cpp's alone."""
    for name in FAMILY_FILES:
        src = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r'getenv\("(\w+)"\)', src):
            assert m.group(1) in ("TC_G16_ABLATE", "TC_G8_ABLATE"), f"{name} reads {m.group(1)}"
        assert src.count("getenv(") == len(re.findall(r'getenv\("TC_G(16|8)_ABLATE"\)', src)), name
        assert not re.search(r"\bdry\b", src) and "sws[" not in src and "_try(" not in src, name
    gen = _gen()
    table = open(os.path.join(CSRC, "gemm_route.cpp")).read()
    for sw in gen.SWITCHES:
        assert table.count(f'"{sw}"') == 1, f"{sw} must be named exactly once, in the switch table"
