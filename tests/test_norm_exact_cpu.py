"""tests/norm_exact_cases.py without a GPU: gn_path() sends every GroupNorm shape down the path the table declares and every
path is present; every case meets the conditions its exactness rests on; the float64 expectation equals the closed form of
its family (A: the integer +-gamma + beta, C: sqrt(N - 1) and -1 / sqrt(N - 1), B: probes at -gamma rstd / N, S: bf16(1 / k));
the probes of the two B seeds and the spikes of the C launches leave no position out; the plain torch statements of the
operators pass every case as they are and, with a seeded defect, are flagged by the family the table names, on every shape
where the defect can occur (the matrix is printed: pytest -s)."""
import pytest
import torch

import norm_exact_cases as X

F64 = torch.float64


@pytest.fixture(scope="module")
def built():
    """name -> (inputs, expected) of launch 0: computed once, never modified"""
    cache = {}

    def get(c):
        if c.name not in cache:
            inp = X.inputs(c)
            cache[c.name] = (inp, X.expected(c, inp))
        return cache[c.name]
    return get


def test_gn_path_sends_every_shape_where_the_table_says():
    seen = set()
    for (s, r, c), label in X.GN_SHAPES:
        p = X.gn_path(s, r, c)
        assert p.label == label, ((s, r, c), p)
        assert s * r * c * 2 <= 2 << 20
        seen.add(label)
    assert seen == {"gn_onepass<256,4>", "gn_onepass<256,13>", "three: gu>4", "three: slab too tall", "three: two slots"}
    g = {shape: X.gn_path(*shape) for shape, _ in X.GN_SHAPES}
    # the particulars the table's comments promise
    assert (g[(3, 70, 320)].vu, g[(3, 70, 320)].rpp) == (5, 51) and 70 % 51
    assert g[(2, 1000, 64)].vu == 1 and 3 * 256 < 1000 < 4 * 256
    assert g[(5, 7, 960)].vu == 15 and 256 - 15 * g[(5, 7, 960)].rpp == 1 and 7 < g[(5, 7, 960)].rpp
    assert 13 * g[(1, 221, 960)].rpp == 221 and (g[(1, 325, 2560)].vu, 13 * g[(1, 325, 2560)].rpp) == (10, 325)
    p = g[(2, 37, 96)]
    assert (p.rows_pp, p.chunk_rows, 37 - (p.nchunks - 1) * p.chunk_rows) == (21, 8, 5)
    assert g[(2, 230, 960)].rows_pp == 2
    p = g[(1, 700, 1280)]
    assert (p.rows_pp, p.nchunks, 700 - (p.nchunks - 1) * p.chunk_rows) == (1, 88, 4) and p.nchunks > 64
    assert g[(1, 330, 2560)].slots == 2 and 256 < 2560 // 8 < 512 and g[(1, 216, 4096)].slots == 2 and 4096 // 8 == 512
    # LayerNorm: three widths or more per instance, no row count a multiple of the rows per block or per wave
    for inst, widths in (((1, 4), (8, 64, 328, 512)), ((2, 2), (520, 1024)), ((4, 1), (1032, 1280, 2048))):
        assert all(X.ln_instance(w) == inst for w in widths)
    assert set(X.LN_WIDTHS) == {8, 64, 328, 512, 520, 1024, 1032, 1280, 2048} and set(X.LN_ROWS) == {1, 5, 18, 33}
    assert all(r % rpb for r in X.LN_ROWS for rpb in (4, 8, 16)) and all(r % 2 or r % 4 for r in X.LN_ROWS)


def test_the_table_holds_every_family_on_every_shape():
    have = {(c.op, c.samples, c.rows, c.c, c.family, c.silu, c.eps, c.seed) for c in X.CASES}
    for (s, r, c), _ in X.GN_SHAPES:
        for eps in X.EPS:
            assert ("groupnorm", s, r, c, "A", False, eps, 0) in have and ("groupnorm", s, r, c, "A", True, eps, 0) in have
        assert {k[7] for k in have if k[:5] == ("groupnorm", s, r, c, "B")} == {0, 1}
        assert any(k[:5] == ("groupnorm", s, r, c, "C") for k in have)
    for w in X.LN_WIDTHS:
        for r in X.LN_ROWS:
            assert {k[6] for k in have if k[:5] == ("layernorm", 1, r, w, "A")} == set(X.EPS)
            assert {k[7] for k in have if k[:5] == ("layernorm", 1, r, w, "B")} == {0, 1}
            assert any(k[:5] == ("layernorm", 1, r, w, "C") for k in have)
    assert len({c.name for c in X.CASES}) == len(X.CASES)
    assert {c.eps for c in X.CASES if c.family == "B"} == set(X.EPS) == {c.eps for c in X.CASES if c.family == "C"}


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_case_is_sound_and_its_expected_value_is_the_closed_form(c, built):
    inp, want = built(c)
    assert X.validate(c, inp) == []
    assert torch.isfinite(want).all()
    ref = X.norm_ref(c, inp)
    if c.family == "A":
        form = X.closed_form(c, inp)
        # the float64 operator differs from the integer by eps alone: < 1e-5 of gamma / d^2, and it rounds to the integer
        assert float((ref - form).abs().max()) < 1e-4
        if c.rule == "equal":
            assert X.differences(c, X.rne_bf16(ref), form) is None
        assert (c.rule == "equal") == (not c.silu and c.shape_key != X.ODD_N_SHAPE) and (c.n % 2 == 1) == (c.shape_key == X.ODD_N_SHAPE)
        assert X.differences(c, X.rne_bf16(ref), want) is None
    elif c.family == "C":
        for launch in sorted({0, X.launches(c) - 1}):
            inp_l = X.inputs(c, launch)
            assert X.validate(c, inp_l) == []
            ref, form = X.norm_ref(c, inp_l), X.closed_form(c, inp_l)
            assert bool(((ref - form).abs() <= 1e-4 * form.abs()).all())        # eps against var = H^2 (N - 1) / N^2 >= 0.59
            s, r, ng = c.geo
            empty = X.to_groups(inp_l["x"], s, r, ng).sum(1) == 0
            assert bool((X.to_groups(ref, s, r, ng)[empty] == 0).all())
    else:
        s, r, ng = c.geo
        v, y = X.to_groups(inp["x"], s, r, ng), X.to_groups(ref / inp["gamma"], s, r, ng)
        var = (v * v).sum(1, keepdim=True) / c.n - 1.0 / c.n ** 2
        probe = (-1.0 / c.n) / torch.sqrt(var + c.eps)
        assert bool(((y - probe).abs()[v == 0] <= 1e-12 * probe.abs().max()).all()) and bool((ref[inp["x"] == 0] != 0).all())
    # the plain statement of the operator, as the kernels build it, passes the case as it stands
    assert X.judge(c, X.norm_model(c, inp), want) is None


def test_family_b_leaves_no_position_out(built):
    for shape in sorted({c.shape_key for c in X.CASES}):
        pair = [c for c in X.CASES if c.family == "B" and c.shape_key == shape]
        assert len(pair) == 2
        x0, x1 = (built(c)[0]["x"] for c in pair)
        assert bool(((x0 != 0) | (x1 != 0)).all()), shape


def test_family_c_carries_the_spike_through_every_row_and_channel():
    by_width = {}
    for c in X.CASES:
        if c.family != "C":
            continue
        plan = X.c_plan(c)
        s, r, ng = c.geo
        rows, chans, empties = set(), set(), 0
        for launch in plan:
            assert len(launch) == s and all(len(spikes) == ng for spikes in launch)
            for i, spikes in enumerate(launch):
                for g, sp in enumerate(spikes):
                    if sp is None:
                        empties += 1
                        continue
                    assert 0 <= sp[0] < r and sp[1] // (c.c // ng) == g       # inside its own sample and group
                    rows.add(sp[0] if c.op == "groupnorm" else i)
                    chans.add(sp[1])
        assert rows == set(range(c.rows)), c.name
        assert empties > 0, c.name
        if c.op == "groupnorm":
            assert chans == set(range(c.c)), c.name
        else:
            by_width.setdefault(c.c, set()).update(chans)
        print(f"{c.name}: {len(plan)} launches")
    for w in X.LN_WIDTHS:
        assert by_width[w] == set(range(w)), w


def _first_of_each_shape(op, family):
    out = {}
    for c in X.CASES:
        if c.op == op and c.family == family:
            out.setdefault(c.shape_key, []).append(c)
    # family B: both seeds of a shape (a defect on one element may fall on a probe in one of them); else the first case
    return [cs if family == "B" else cs[:1] for cs in out.values()]


def _c_launch_for(c, defect):
    """family C: a launch in which the element the defect concerns (GroupNorm: the last row, LayerNorm: the last vector)
    carries the spike.  The LayerNorm cases of fewer than 33 rows run 8 launches and need not have one: None"""
    for launch, plan in enumerate(X.c_plan(c)):
        for spikes in plan:
            for sp in spikes:
                if sp is not None and (sp[0] == c.rows - 1 if c.op == "groupnorm" else sp[1] >= c.c - 8):
                    return launch
    assert c.op == "layernorm" and c.rows != max(X.LN_ROWS), f"{c.name}: no launch puts the spike where {defect} looks"
    return None


def test_every_seeded_defect_is_flagged_by_its_family_on_every_shape_where_it_can_occur(built):
    missing = []
    for defect, (ops, family) in X.DEFECTS.items():
        for op in ops:
            flagged = shapes = 0
            for group in _first_of_each_shape(op, family):
                if not X.occurs(defect, group[0]) or (family == "C" and _c_launch_for(group[0], defect) is None):
                    continue
                shapes += 1
                hit = False
                for c in group:
                    if c.family == "C":
                        inp = X.inputs(c, _c_launch_for(c, defect))
                        want = X.expected(c, inp)
                    else:
                        inp, want = built(c)
                    assert X.judge(c, X.norm_model(c, inp), want) is None
                    hit = hit or X.judge(c, X.norm_model(c, inp, defect), want) is not None
                flagged += hit
                if not hit:
                    missing.append((defect, group[0].shape_key))
            print(f"{defect} / {op}: family {family} flags {flagged} of {shapes} shapes")
            assert shapes, (defect, op)
    assert not missing, f"defects their family does not see: {missing}"


def test_the_defect_by_family_matrix(built):
    """which family sees which defect, on one GroupNorm shape per path and three LayerNorm shapes.  Pinned in both directions
    where the construction decides it: `must` (the family is there for it) and `must_not` (the family cannot see it: B and C
    have beta = 0, C has gamma = 1, and B's and C's means are 1 / N and H / N, nothing beside their variance), so that a change
    of the input families that blinds one of them -- or a judge that flags everything -- shows here"""
    shapes = ("groupnorm-3x70x320", "groupnorm-2x300x320", "groupnorm-2x37x96", "groupnorm-2x230x960", "groupnorm-1x330x2560",
              "layernorm-1x33x328", "layernorm-1x33x1024", "layernorm-1x33x1280")
    must = {
        "drop_chunk_last_row": {"B"}, "drop_vector": {"B"}, "double_count": {"B"}, "stats_next_group": {"A"},
        "stats_next_sample": {"A"}, "gamma_shift8": {"A", "B"}, "beta_shift8": {"A"}, "pad_in_var": {"A"},
        "spike_not_in_var": {"C"}, "store_past_tail": {"A", "B", "C"},
    }
    must_not = {"beta_shift8": {"B", "C"}, "gamma_shift8": {"C"}, "pad_in_var": {"B", "C"}}
    assert set(must) == set(X.DEFECTS) and all(X.DEFECTS[d][1] in must[d] for d in must)
    for defect in X.DEFECTS:
        every, never = set(), set()
        for family in "ABC":
            hits = []
            for key in shapes:
                group = [c for c in X.CASES if c.shape_key == key and c.family == family and not c.silu]
                group = group if family == "B" else group[:1]
                if not X.occurs(defect, group[0]):
                    continue
                hit = False
                for c in group:
                    if family == "C":
                        inp = X.inputs(c, _c_launch_for(c, defect))
                        wanted = X.expected(c, inp)
                    else:
                        inp, wanted = built(c)
                    hit = hit or X.judge(c, X.norm_model(c, inp, defect), wanted) is not None
                hits.append(hit)
            if hits and all(hits):
                every.add(family)
            if hits and not any(hits):
                never.add(family)
        print(f"{defect}: flagged on every shape by {sorted(every)}, on none by {sorted(never)}")
        assert must[defect] <= every, (defect, every)
        assert must_not.get(defect, set()) <= never, (defect, never)


def test_a_report_names_the_groups_and_the_residues(built):
    c = next(c for c in X.CASES if c.name == "gn-3x70x320-A-eps1e-05")
    inp, want = built(c)
    msg = X.judge(c, X.norm_model(c, inp, "stats_next_group"), want)
    assert msg is not None and "gn_onepass<256,4>" in msg and "(sample, group): [(0, 0), (0, 1)" in msg and "channels mod 8" in msg
    msg = X.judge(c, X.norm_model(c, inp, "store_past_tail"), want)
    assert "rows behind the output were written: output rows + [0]" in msg
    assert "shape" in X.differences(c, want[:-1], want)
    # a NaN and a value just beyond one ulp fail; one ulp passes; an expected zero admits nothing but zero
    ref = torch.tensor([[1.0, 1.5, 0.0, -3.0]], dtype=F64)
    cc = X.Case("t", "layernorm", "B", 1, 1, 4)
    ulp = X.bf16_ulp(ref)
    assert ulp.tolist() == [[2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -6]]
    assert X.differences(cc, ref + ulp, ref) is None and X.differences(cc, ref - ulp, ref) is None
    for k in (0, 1, 3):
        bad = ref.clone()
        bad[0, k] += 1.01 * float(ulp[0, k])
        assert X.differences(cc, bad, ref) is not None
    bad = ref.clone()
    bad[0, 2] = 1e-30
    assert "want exact 0" in X.differences(cc, bad, ref)
    bad[0, 2] = float("nan")
    assert X.differences(cc, bad, ref) is not None


@pytest.mark.parametrize("c,prows", X.PART_CASES, ids=lambda v: v.name if isinstance(v, X.Case) else str(v))
def test_groupnorm_from_partial_sums_and_one_poisoned_partial(c, prows):
    inp = X.inputs(c)
    assert X.validate(c, inp) == [] and c.rows % prows == 0
    part = X.exact_part(inp["x"], prows)
    assert tuple(part.shape) == (c.total_rows // prows, 2, c.c) and (c.rows // prows > 256 or prows == c.rows)
    want = X.expected(c, inp)
    assert X.differences(c, X.rne_bf16(X.gn_from_part(c, inp, part, prows)), want) is None
    for blk, which, ch in ((0, 0, 0), (part.shape[0] - 1, 0, c.c - 1), (part.shape[0] // 2, 0, 33)):
        bad = part.clone()
        bad[blk, which, ch] += 1
        msg = X.differences(c, X.rne_bf16(X.gn_from_part(c, inp, bad, prows)), want)
        assert msg is not None, (blk, which, ch)
        sample, group = blk * prows // c.rows, ch // (c.c // 32)
        assert f"(sample, group): [({sample}, {group})] (1 in all)" in msg, msg


# ------------------------------------------------------------------------------------------------------------------ softmax
def test_softmax_table():
    kinds = {(c.kind, c.n) for c in X.SCASES if not c.n_out}
    assert {("onehot", n) for n in (1, 255, 256, 257, 2560)} <= kinds and all(c.rows == c.n for c in X.SCASES if c.kind == "onehot")
    eq = [c for c in X.SCASES if c.kind == "equal" and not c.n_out]
    assert eq and all(c.rows == c.n >= 64 for c in eq)          # row r's set holds column r: every column is in some set
    assert any(c.causal_period == 77 and c.rows == 3 * 77 for c in X.SCASES)
    dims = {c.dims for c in X.SCASES if c.n_out}
    assert (77, 80, 88, 96) in dims and any(d[0] == 257 and d[1] == 264 and d[3] > 264 and d[2] > 257 for d in dims)
    # fl32(1 / k) lies farther than 2^-21 (relative) from every bf16 tie: neither a 1-ulp reciprocal nor a 1-ulp exp moves it
    m = X.recip_margin()
    print(f"min relative distance of fl32(1/k), k = 1 .. 2560, from a bf16 tie: {m:.3e}")
    assert m > 2.0 ** -21


@pytest.mark.parametrize("c", X.SCASES, ids=lambda c: c.name)
def test_softmax_closed_form_and_defects(c):
    s = X.s_inputs(c)
    n, n_out, lds, ldo = c.dims
    assert tuple(s.shape) == (c.rows, lds) and bool((s[:, n:] == X.POISON).all())
    want = X.s_closed_form(c)
    assert float(want[:c.rows, :n].sum(1).sub(1).abs().max()) < 2.0 ** -7       # rows of bf16(1 / k) sum to 1 within k roundings
    assert X.s_judge(c, X.softmax_model(c, s), want) is None
    if c.kind == "equal":
        cover = set()
        for r in range(c.rows):
            cover.update(X._s_set(c, r))
        assert cover == set(range(n))
    for defect, kind in X.S_DEFECTS.items():
        concerned = ("strides" in c.name) if kind == "strides" else (c.kind == kind)
        if defect == "sum_miss_col":
            concerned = concerned and c.rows >= c.n
        if not concerned:
            continue
        msg = X.s_judge(c, X.softmax_model(c, s, defect), want)
        assert msg is not None, defect
        print(f"{c.name} / {defect}: {msg[:160]}")


def test_every_softmax_defect_has_a_case():
    for defect, kind in X.S_DEFECTS.items():
        assert any(("strides" in c.name) if kind == "strides" else (c.kind == kind) for c in X.SCASES), defect
