"""Every route of a transformer block, recorded before the routing moved into one if-chain per sub-layer and reproduced
after: tests/golden/block_routes.json holds, per case, the operator calls one BasicTransformerBlock makes on the emulated
contract (names, operand shapes / strides / dtypes / value digests, scalars) and its output, taken from the parent commit
by tests/golden/make_block_routes.py.  This tree must give the same text byte for byte, and ask each eligibility rule at
most once per sub-layer (the parent asked ff_fused_eligible twice).  CPU only, no library."""
import importlib.util
import json
import os
import re

import pytest

from conftest import ROOT

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
COVERAGE = ("layernorm", "gemm", "gemm_ln", "attention", "attention_temporal", "attention_temporal_rel", "temporal_qkv_attn",
            "temporal_attn_fused", "ff_geglu_fused")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_block_routes", os.path.join(GOLDEN_DIR, "make_block_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(gen):
    with open(gen.GOLDEN) as f:
        return f.read()


@pytest.fixture(scope="module")
def recorded(gen):
    return gen.record(ROOT)


def test_golden_covers_every_route(gen, golden):
    g = json.loads(golden)
    names = [n for n, *_ in gen.cases()]
    assert list(g["cases"]) == names and len(names) == 88 and set(g["full"]) == set(gen.FULL) <= set(names)
    assert len({v[0] for v in g["cases"].values()}) == 17
    seen = {op for v in g["cases"].values() for op in v[0].split()}
    for op in COVERAGE:
        assert op in seen, op
    for k, lines in g["full"].items():
        assert " ".join(gen.op_name(l) for l in lines) == g["cases"][k][0] and gen.digest(lines) == g["cases"][k][1]
    # a folded weight is told from a plain one: the weight (second operand) of a GEMM that normalises its rows occurs
    # nowhere in the same block's calls without the fold
    plain = "".join(g["full"]["temporal plain ln=None ff=None tb=None tqa=True"])
    folded = [re.findall(r"#[0-9a-f]{12}", l)[1] for l in g["full"]["temporal plain ln=64 ff=None tb=None tqa=True"] if "a_norm_eps=" in l]
    assert len(folded) == 3 and not any(d in plain for d in folded)


def test_mx_stand_in_reaches_gemm_only(golden):
    """A LayerNorm output that is not a tensor (ops.MxRows on the fp8 route) goes to its one consumer GEMM, never to the
    one-launch qkv + attention, which reads bf16 rows -- although that route is on offer."""
    g = json.loads(golden)
    k = "temporal plain ln=None ff=None tb=None tqa=True"
    assert g["cases"][k][0].count("temporal_qkv_attn") == 2 and g["cases"][k + " mx"][0].count("temporal_qkv_attn") == 0
    lines = g["full"][k + " mx"]
    takers = [l[:l.index("(")] for l in lines if "Mx(" in l]
    assert takers == ["gemm"] * 3 and all(l.startswith("gemm(Mx(") for l in lines if "Mx(" in l)
    assert not any("Mx(" in l for key, ls in g["full"].items() if not key.endswith(" mx") for l in ls)


def test_this_tree_reproduces_the_golden_byte_for_byte(gen, golden, recorded, tmp_path):
    got = gen.dumps(recorded)
    if got != golden:
        (tmp_path / "got.json").write_text(got)
        want = json.loads(golden)["cases"]
        moved = [k for k, v in recorded.items() if [v["ops"], gen.digest(v["lines"]), v["out"]] != want.get(k)]
        pytest.fail(f"{len(moved)} cases differ from tests/golden/block_routes.json, first: {moved[:3]} (this tree's text: "
                    f"{tmp_path / 'got.json'}; every line of a tree: tests/golden/make_block_routes.py --tree DIR --text FILE)")


def test_every_rule_is_asked_at_most_once_per_sub_layer(gen, recorded):
    asked = set()
    for name, v in recorded.items():
        assert all(n <= 1 for n in v["probes"].values()), (name, v["probes"])
        asked |= set(v["probes"])
    assert asked == set(gen.RULES)
