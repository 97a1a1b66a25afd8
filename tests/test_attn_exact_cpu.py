"""tests/attn_exact_cases.py without a GPU: every case meets the conditions its exactness rests on, the float64 expected value
equals the closed form (v[pi] + what the operator adds, c, the bf16(1/n) formula), the project's own CPU statements of the
operators (tests/emu_ops.py, tests/relpos_cases.py, tests/q8_attn_ref.py) give the same bits, and every seeded defect changes
the expected output of at least one case of each operator it concerns (the lists are printed: pytest -s)."""
import pytest
import torch

import attn_exact_cases as X

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def built():
    """name -> (inputs, expected): computed once, never modified"""
    cache = {}

    def get(c):
        if c.name not in cache:
            inp = X.inputs(c)
            cache[c.name] = (inp, X.expected(c, inp))
        return cache[c.name]
    return get


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_case_is_sound_and_its_expected_value_is_the_closed_form(c, built):
    inp, want = built(c)
    assert X.validate(c, inp) == []
    form = X.closed_form(c, inp)
    assert X.differences(c, want, form, inp) is None
    assert torch.isfinite(want.float()).all()


def test_midpoint_margin():
    """1 / n, n = 1 .. 64, against the bf16 rounding midpoints: the nearest is 2^-11 away or more, the reciprocal instruction's
    error is 2^-23"""
    assert X.midpoint_margin() > 2.0 ** -20
    print(f"min relative distance of 1/n from a bf16 midpoint: {X.midpoint_margin():.3e}")


def test_the_table_holds_every_operator_with_every_construction():
    have = {(c.op, c.target.split("<")[0], c.kind) for c in X.CASES}
    for op, kernel in (("attention", "attn_d64_dma_kernel"), ("attention_q8", "attn_d64_q8_kernel"), ("temporal", "attn_temporal_kernel"),
                       ("temporal", "attn_temporal_long_kernel"), ("temporal_rel", "attn_temporal_rel_kernel")):
        for kind in ("gather", "equal"):
            assert (op, kernel, kind) in have, (op, kernel, kind)
    assert ("temporal_rel", "attn_temporal_rel_kernel", "gather_dist") in have
    for op, kernel in (("qkv_attn", "qkv_attn_kernel"), ("qkv_attn", "qkv_attn_long_kernel"), ("tb_fused", "tb_fused_kernel")):
        assert (op, kernel, "gather") in have
    targets = {c.target for c in X.CASES}
    assert {"attn_d64_dma_kernel<false>", "attn_d64_dma_kernel<true>"} <= targets
    for tt, w in ((32, 4), (64, 2)):
        assert {f"attn_temporal_long_kernel<{tt}>", f"qkv_attn_long_kernel<{tt}>", f"attn_temporal_rel_kernel<{tt}, {w}, true>",
                f"attn_temporal_rel_kernel<{tt}, 4, false>"} <= targets
    # the register-staged arm runs the non-dual attention cases: both constructions, accumulate, packed, shared K/V
    reg = X.REG_CASES
    assert {c.kind for c in reg} == {"gather", "equal"} and any(c.accumulate for c in reg) and any(c.packed for c in reg) \
        and any(c.kv_bdiv == 2 for c in reg)
    dual = [c for c in X.CASES if c.lk2]
    assert {c.kind for c in dual} == {"gather", "equal"} and any(c.accumulate for c in dual)
    sp = [c for c in X.CASES if c.op == "attention" and not c.lk2]
    assert {c.lq for c in sp} == {1, 33, 128, 129, 200} and {c.lk for c in sp} == {1, 31, 64, 65, 77, 129, 200}
    assert {c.heads for c in sp} == {1, 2, 3} and any(c.batch == 3 and c.kv_bdiv == 2 for c in sp)
    rel = [c for c in X.CASES if c.op == "temporal_rel" and c.tables and not c.zero_tables]
    assert {(c.t, c.max_rel == c.t, c.causal, c.kind) for c in rel} == \
        {(t, full, causal, kind) for t in (6, 17, 33, 64) for full in (False, True) for causal in (False, True) for kind in ("gather", "gather_dist")}


def _emu_output(c, inp):
    """the case through the project's CPU statement of its operator"""
    from emu_ops import EmuOps
    from relpos_cases import RelEmuOps
    emu = RelEmuOps(round_bf16=True, tqa=True, tb_fused_c=c.heads * 64)
    t16 = {k: v.to(BF16) for k, v in inp.items() if k in ("q", "k", "v", "k2", "v2", "base", "qkv", "rel_k", "rel_v", "x")}
    if c.op == "attention":
        kw = dict(batch=c.batch, heads=c.heads, lq=c.lq, lk=c.lk, kv_bdiv=c.kv_bdiv)
        if c.lk2:
            kw.update(k2=t16["k2"], v2=t16["v2"], lk2=c.lk2, kv2_bdiv=c.kv2_bdiv)
        out = t16["base"].clone() if c.accumulate else None
        return emu.attention(t16["q"], t16["k"], t16["v"], out=out, accumulate=c.accumulate, **kw)
    if c.op == "attention_q8":
        import q8_attn_ref
        return q8_attn_ref.attention_rows(t16["q"], t16["k"], t16["v"], batch=c.batch, heads=c.heads, lq=c.lq, lk=c.lk, scale=X.SCALE).to(BF16)
    kw = dict(b=c.batch, t=c.t, hw=c.hw, heads=c.heads)
    if c.op == "temporal":
        return emu.attention_temporal(t16["qkv"], **kw)
    if c.op == "temporal_rel":
        return emu.attention_temporal_rel(t16["qkv"], t16.get("rel_k"), t16.get("rel_v"), max_rel=c.max_rel, causal=c.causal, **kw)
    w, bq = inp["wqkv"].to(BF16), inp["bqkv"].float()
    if c.op == "qkv_attn":
        return emu.temporal_qkv_attn(t16["x"], w, bq, **kw)
    return emu.temporal_attn_fused(t16["x"], w, bq, inp["wo"].to(BF16), inp["bo"].float(), ln_eps=None, **kw)


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_the_cpu_statements_of_the_operators_give_the_same_bits(c, built):
    inp, want = built(c)
    got = _emu_output(c, inp)
    if c.kind == "equal" and c.family == "mfma" and (c.causal or c.t & (c.t - 1)):
        # equal weights on an MFMA core where n is no power of two: the kernel's documented bf16 weight gives bf16(1 / n) n != 1,
        # which the fp32-weight statement does not model.  The two then differ by that one rounding (2^-9 of the mean |v|, and
        # |v| <= 14) and the two stores' (2^-9 of the result each), no more
        g, w = got.double(), want.double()
        assert float(inp["vseq"].abs().max()) <= 14 and bool(((g - w).abs() <= 3 * 2.0 ** -9 * 14).all())
        return
    assert X.differences(c, got, want, inp) is None


def test_every_seeded_defect_changes_a_case_of_each_operator_it_concerns(built):
    missing = []
    for defect, ops in X.DEFECTS.items():
        for op in ops:
            caught = []
            for c in X.CASES:
                if c.op != op:
                    continue
                inp, want = built(c)
                broken = X.expected(c, inp, defect=defect)
                if X.differences(c, broken, want) is not None:
                    caught.append(c.name)
            print(f"{defect} / {op}: {len(caught)} cases: {', '.join(caught)}")
            if not caught:
                missing.append((defect, op))
    assert not missing, f"defects no case sees: {missing}"


def test_a_gather_report_names_the_key_that_arrived(built):
    c = next(c for c in X.CASES if c.name == "attn-gather-200x200-b1h2")
    inp, want = built(c)
    msg = X.differences(c, X.expected(c, inp, defect="swap_p"), want, inp)
    assert msg is not None and "got the V row of key" in msg and "target keys mod 16" in msg and "queries mod 128" in msg
    # every differing query's target sits in slots 4..11 of its 16-key step, and the report says so
    assert "target keys mod 16: [4, 5, 6, 7, 8, 9, 10, 11]" in msg, msg
    short = X.differences(c, want[:-1], want, inp)
    assert "shape" in short
