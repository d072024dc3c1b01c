"""CPU checks of tests/_solve_ref.py: the case table crosses every edge it names (recomputed from the shapes), the data of every case
factorise and leave no tile negligible, the long-double references are not what the bounds measure (float64 evaluation stays within 1/8 of
every bound), and the measures of tests/test_gpu_solve_edges.py see each simulated fault at 10x its bound at least."""
import numpy as np
import pytest

from tests import _solve_ref as R

pytestmark = pytest.mark.skipif(not R.HAS_LONGDOUBLE, reason="numpy's longdouble is no wider than float64 here")

MATERN = ("matern52", "matern32", "exponential")

# edge -> what the shapes and options of a case that claims it must show
EDGES = {
    "M5": lambda c, f: c["M"] == 5 and f["Mp"] == 32 and f["nct"] == 1,
    "M33": lambda c, f: c["M"] == 33 and f["Mp"] == 64,
    "M65": lambda c, f: c["M"] == 65 and f["Mp"] == 96 and (c["ctx"] == "pure" or (f["half_tile"] and f["ke_capped"])),
    "M129": lambda c, f: c["M"] == 129 and f["Mp"] == 160,
    "M250": lambda c, f: c["M"] == 250 and f["Mp"] == 256 and (f["nct"] == 4 or c["ctx"] == "pure"),
    "M257": lambda c, f: c["M"] == 257 and f["Mp"] == 288,
    "M512": lambda c, f: c["M"] == 512 and f["vpr"] == (128 if c["ctx"] == "pure" else 256) and f["nct"] == (4 if c["ctx"] == "pure" else 8),
    "M513": lambda c, f: c["M"] == 513 and f["Mp"] == 544,
    "n1": lambda c, f: c["n"] == 1, "n127": lambda c, f: c["n"] == 127, "n128": lambda c, f: c["n"] == 128 and f["last_rows"] == 128,
    "n129": lambda c, f: c["n"] == 129 and f["last_rows"] == 1,
    "n1025": lambda c, f: c["n"] == 1025 and f["rtiles"] == 9 and f["last_rows"] == 1,
    "n_cap": lambda c, f: f["ldk"] != c["n"] and c["n_cap"] > c["n"],
    "D1": lambda c, f: c["D"] == 1, "D2": lambda c, f: c["D"] == 2 and f["dd"] == 2, "D3": lambda c, f: c["D"] == 3 and f["dd"] == 4,
    "D4": lambda c, f: c["D"] == 4 and f["dd"] == 4,
    "serpentine": lambda c, f: c["ctx"] != "pure" and f["serpentine"] and f["nct"] >= 4,
    "serpentine32": lambda c, f: c["ctx"] == "pure" and f["serpentine"] and f["nct"] >= 4,
    "round2": lambda c, f: f["round2"] and f["grid"] == 16 * f["nct"],
    "ragged": lambda c, f: c["n"] % R.TILE != 0,
    "rmax": lambda c, f: c["n"] % R.TILE != 0 and c["ctx"] != "pure" and f["epilogue"] == "lds",
    "rpp1": lambda c, f: f["rbf_f64"] and f["rpp"] == 1,
    "idle_threads": lambda c, f: f["rbf_f64"] and f["rpp"] == 5 and f["idle_threads"],
    "wide_rows": lambda c, f: c["ctx"] != "pure" and f["wide_rows"] and not f["rbf_f64"],
    "rbf_dd4": lambda c, f: f["rbf_f64"] and f["dd"] == 4,
    "root": lambda c, f: c["ctx"] == "f64" and c["kind"] in MATERN,
    "tri1": lambda c, f: f["last_chunk_valid"] and f["nct"] >= 2,
    "tri2": lambda c, f: f["last_chunk_valid"] and f["nct"] >= 2,
    "f16x3": lambda c, f: c["ctx"] == "f32" and "mfma_mode" not in c["opts"],
    "bf16x6": lambda c, f: c["ctx"] == "f32" and c["opts"].get("mfma_mode") == "bf16x6",
    "pure": lambda c, f: c["ctx"] == "pure" and f["cw"] == 128 and f["bk"] == 32,
    "lz": lambda c, f: c["opts"].get("learn_inducing") and f["epilogue"] == "generic",
    "ard": lambda c, f: c["opts"].get("ard"),
    "periodic": lambda c, f: c["kind"] == "periodic" and c["ctx"] == "f64" and f["D"] == 2 and f["epilogue"] == "lds",
    "product": lambda c, f: c["kind"] == "product" and c["ctx"] == "f64" and f["D"] == 3 and f["epilogue"] == "generic",
    "hyper_tn": lambda c, f: c["opts"].get("hyper_tn") and c["ctx"] == "f32" and c["kind"] not in ("rationalquadratic", "periodic", "product")
    and not c["opts"].get("ard") and not c["opts"].get("learn_inducing") and f["dk_rpp"] >= 1,
    "dk_rpp3": lambda c, f: c["opts"].get("hyper_tn") and f["dk_rpp"] == 3,
    "K1": lambda c, f: c["K"] == 1,
}
EVERY_M, EVERY_N = (5, 33, 65, 129, 250, 257, 512, 513), (1, 127, 128, 129, 1025)


def test_case_table_crosses_every_named_edge():
    assert 35 <= len(R.CASES) <= 45
    claimed = set()
    for name, c in R.CASES.items():
        f = R.facts(c)
        for e in c["edges"]:
            assert EDGES[e](c, f), (name, e, f)
            claimed.add(e)
    assert claimed == set(EDGES), set(EDGES) - claimed
    cs = [(c, R.facts(c)) for c in R.CASES.values()]
    some = lambda pred: any(pred(c, f) for c, f in cs)
    # every M and n, in both solve types where the type changes the tiling
    assert {c["M"] for c, _ in cs} == set(EVERY_M) and {c["n"] for c, _ in cs} == set(EVERY_N)
    for M in (129, 512, 513):
        assert some(lambda c, f: c["M"] == M and c["ctx"] == "pure") and some(lambda c, f: c["M"] == M and c["ctx"] == "f32")
    # all five kinds on the K_nm kernels of every context type, and the RBF f64 kernel in its DD = 2, DD = 4 and ARD instantiations
    for ctx in ("f64", "f32", "pure"):
        assert {c["kind"] for c, _ in cs if c["ctx"] == ctx} >= set(R.KINDS), ctx
    for dd in (2, 4):
        assert some(lambda c, f: f["rbf_f64"] and f["dd"] == dd and not c["opts"].get("ard") and c["kind"] == "rbf")
    assert some(lambda c, f: f["rbf_f64"] and c["opts"].get("ard")) and some(lambda c, f: not f["rbf_f64"] and c["opts"].get("ard"))
    # the backward: both epilogues of the f64 solve, their ARD and periodic variants, with and without learnable inducing inputs
    for ep in ("lds", "generic"):
        assert some(lambda c, f: c["ctx"] != "pure" and f["epilogue"] == ep and not c["opts"].get("ard") and c["kind"] in R.KINDS)
        assert some(lambda c, f: c["ctx"] != "pure" and f["epilogue"] == ep and c["opts"].get("ard"))
    assert some(lambda c, f: c["opts"].get("ard") and c["opts"].get("learn_inducing"))
    # the edges of the LDS-transposed epilogue: rmax (a ragged last row tile), cok (padded columns), ncl (a lane's pair past Mp: a half-filled
    # last column tile), padding workgroups of the XCD grid
    lds = lambda c, f: c["ctx"] != "pure" and f["epilogue"] == "lds"
    assert some(lambda c, f: lds(c, f) and c["n"] % R.TILE != 0) and some(lambda c, f: lds(c, f) and c["M"] < f["Mp"])
    assert some(lambda c, f: lds(c, f) and f["half_tile"]) and some(lambda c, f: lds(c, f) and f["padding_blocks"] > 0)
    # the map: a second round with and without the serpentine, in both solve types
    assert some(lambda c, f: f["round2"] and f["serpentine"] and c["ctx"] != "pure") and some(lambda c, f: f["round2"] and not f["serpentine"])
    assert some(lambda c, f: f["round2"] and f["serpentine"] and c["ctx"] == "pure")
    # red_d[6] is non-zero for RationalQuadratic only: it is there in every context type and with learnable inducing inputs
    assert some(lambda c, f: c["kind"] == "rationalquadratic" and c["opts"].get("learn_inducing"))
    assert some(lambda c, f: c["n_cap"] > c["n"] and c["ctx"] == "f32") and some(lambda c, f: c["n_cap"] > c["n"] and c["ctx"] == "f64")


@pytest.fixture(scope="module")
def refs():
    """Per case, computed once: the host's operands and the long-double references with their bounds."""
    cache = {}

    def get(name):
        if name not in cache:
            o = R.host_operands(name)
            c = o["case"]
            W, Wb = R.w_ref(c, o["Knm"], o["Linv"])
            Kb, Kbb = R.kbar_ref(c, o["Wbar"], o["Linv"])
            T, P = R.terms(c, o["kn"], o["Knm"])
            cache[name] = dict(o, W=W, W_bound=Wb, Kb=Kb, Kb_bound=Kbb, T=T, P=P, sums=R.sums(c, Kb, Kbb, T, P))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(R.CASES))
def test_data_factorise_and_leave_no_tile_negligible(name, refs):
    r = refs(name)                      # numpy's Cholesky of K_uu + jitter I in the solve precision ran in host_operands
    c = r["case"]
    assert np.isfinite(r["Linv"]).all() and r["Linv"].dtype == np.float64
    shares = R.no_negligible_tile(c, r["W"], r["Kb"], r["T"])
    print(name, {k: "%.1e" % v for k, v in shares.items()})
    for k, v in shares.items():
        assert v >= R.MIN_SHARE, (name, k, v)


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_evaluation_stays_within_an_eighth_of_every_bound(name, refs):
    """Every reference evaluated in float64 instead of long double stays within 1/8 of its bound: the bounds measure the device, not the
    reference.  K_nm under the f64 solve is the one quantity where this cannot hold - the bound there IS the rounding of a float64 evaluation,
    (D + 2) u on r2 and 4 u on the profile, and a float64 restatement spends about a third of it (measured: 0.09 to 0.91) - so there the
    float64 evaluation is held to the bound itself, and the long-double reference to 1/8 of it against a 50-digit evaluation of sampled
    elements (the r2 = 0 element, the largest and smallest k, and random ones)."""
    r = refs(name)
    c, st = r["case"], r["st"]
    t = np.float64
    kn64 = R.knm(c, st["X"], st["Z"], st["params"], t=t)
    out = dict(Knm=R.ratio(kn64["k"], r["kn"]["k"], r["kn"]["bound"]))
    out["W"] = R.ratio(R.w_ref(c, r["Knm"], r["Linv"], t=t)[0], r["W"], r["W_bound"])
    Ws = np.asarray(r["W"], np.float64)
    q, qb = R.q_ref(c, Ws)
    out["q"] = R.ratio(R.q_ref(c, Ws, t=t)[0], q, qb)
    T64, P64 = R.terms(c, kn64, r["Knm"], t=t)
    v64, _ = R.sums(c, R.kbar_ref(c, r["Wbar"], r["Linv"], t=t)[0], r["Kb_bound"], T64, P64)
    val, bnd = r["sums"]
    for k in val:
        out[k] = R.ratio(v64[k], val[k], bnd[k])
    G, Gb = R.gt_ref(c, Ws, r["Wbar"])
    out["GT"] = R.ratio(R.gt_ref(c, Ws, r["Wbar"], t=t)[0], G, Gb)
    # the long-double K_nm against 50 digits
    k = np.asarray(r["kn"]["k"], np.float64)
    rng = np.random.default_rng(3)
    picks = {(0, 0), tuple(int(v) for v in np.unravel_index(k.argmax(), k.shape)), tuple(int(v) for v in np.unravel_index(k.argmin(), k.shape))}
    picks |= {(int(rng.integers(c["n"])), int(rng.integers(c["M"]))) for _ in range(24)}
    picks = sorted(picks)
    exact = R.knm_decimal(c, st["X"], st["Z"], st["params"], picks)
    import decimal
    with decimal.localcontext() as cx:
        cx.prec = 50
        ld = lambda v: decimal.Decimal(float(v)) + decimal.Decimal(float(v - R.LD(float(v))))          # exact: two float64 pieces
        err = [abs(float(ld(r["kn"]["k"][n, j]) - e)) for (n, j), e in zip(picks, exact)]
    out["Knm_ld"] = max(e / float(r["kn"]["bound"][n, j]) if r["kn"]["bound"][n, j] > 0 else (0.0 if e == 0 else np.inf) for (n, j), e in zip(picks, err))
    print(name, {k: "%.3f" % v for k, v in out.items()})
    limit = {k: 0.125 for k in out}
    if c["ctx"] != "pure":
        limit["Knm"] = 1.0
    bad = {k: v for k, v in out.items() if not v <= limit[k]}
    assert not bad, (name, bad)


# ---- sensitivity: every simulated fault exceeds its bound 10x in the measure meant to catch it --------------------------------------------

FACTOR = 10.0


def _claiming(*edges, pred=None):
    return [n for n, c in R.CASES.items() if all(e in c["edges"] for e in edges) and (pred is None or pred(c, R.facts(c)))]


@pytest.mark.parametrize("name", _claiming("tri1"))
def test_a_forward_k_range_one_chunk_short_in_the_last_column_tile(name, refs):
    r = refs(name)
    c, f = r["case"], R.facts(r["case"])
    ct = f["nct"] - 1
    ke = min((ct + 1) * f["cw"], f["Mp"])
    bad, _ = R.w_ref(c, r["Knm"], r["Linv"], ranges={ct: (0, ke - f["bk"])})
    e, t = R.ratio(bad, r["W"], r["W_bound"]), R.tile_ratio(bad, r["W"], r["W_bound"], ct=f["cw"])
    print(name, "elementwise %.2e  per tile %.2e" % (e, t))
    assert e > FACTOR and t > FACTOR


@pytest.mark.parametrize("name", _claiming("tri2"))
@pytest.mark.parametrize("which", ["first", "last"])
def test_a_backward_k_range_starting_one_chunk_late(name, which, refs):
    """Seen in the scalar sums under the f64 solve.  In pure_fp32 contexts the worst-case bound of a scalar sum of n M float32 terms is wider
    than one chunk of one tile: the measure there is G, the per-column sums of a learn_inducing context (the triangular core is the same)."""
    r = refs(name)
    c, f = r["case"], R.facts(r["case"])
    ct = 0 if which == "first" else f["nct"] - 1
    bad, _ = R.kbar_ref(c, r["Wbar"], r["Linv"], ranges={ct: (ct * f["cw"] + f["bk"], c["M"])})
    v, _ = R.sums(c, bad, r["Kb_bound"], r["T"], r["P"])
    val, bnd = r["sums"]
    seen = {k: R.ratio(v[k], val[k], bnd[k]) for k in (("G",) if c["ctx"] == "pure" else ("s1", "s2"))}
    print(name, which, seen)
    assert min(seen.values()) > FACTOR


@pytest.mark.parametrize("name", _claiming("rmax"))
@pytest.mark.parametrize("weight", [0.0, 2.0], ids=["dropped", "twice"])
def test_the_last_valid_row_of_a_ragged_tile_dropped_or_counted_twice(name, weight, refs):
    """The rmax clamp of the LDS-transposed f64 epilogue without its rok mask: the last valid row stands in for the rows past it."""
    r = refs(name)
    c = r["case"]
    rows = np.ones(c["n"])
    rows[-1] = weight
    v, _ = R.sums(c, r["Kb"], r["Kb_bound"], r["T"], r["P"], rows=rows)
    val, bnd = r["sums"]
    names = ["s1"] + (["axis"] if c["opts"].get("ard") or R.sources(c) else ["s2"])
    seen = {k: R.ratio(v[k], val[k], bnd[k]) for k in names}
    print(name, seen)
    assert min(seen.values()) > FACTOR


@pytest.mark.parametrize("name", ["f64_m52_M33_n129_D2", "f64_exp_M129_n127_D4", "f32_rq_M33_n129_D4", "ard_f64_m52_M65_n127_D3", "pure_rq_M65_n128_D4"])
def test_a_padded_column_counted(name, refs):
    """The padded columns of K_nm are zeros, so the sums cannot see them being counted: what catches a kernel that evaluates them (at the
    zero coordinates its registers hold there) is the exact-zero check of the padding, and the value it would find is no rounding error."""
    r = refs(name)
    c, st = r["case"], r["st"]
    assert c["M"] < R.facts(c)["Mp"]
    pad = R.knm(c, st["X"], np.zeros((1, c["D"])), st["params"])["k"]
    assert float(np.abs(pad).max()) > FACTOR * float(r["kn"]["bound"].max())


@pytest.mark.parametrize("name", _claiming("serpentine") + _claiming("serpentine32"))
def test_a_column_tile_swapped_with_its_serpentine_mirror(name, refs):
    r = refs(name)
    c, f = r["case"], R.facts(r["case"])
    bad = np.array(r["W"])
    cw, ct = f["cw"], 1
    mirror = (ct & ~3) + 3 - (ct & 3)
    width = min(cw, c["M"] - mirror * cw)
    bad[:, ct * cw:ct * cw + width], bad[:, mirror * cw:mirror * cw + width] = r["W"][:, mirror * cw:mirror * cw + width], r["W"][:, ct * cw:ct * cw + width]
    assert R.ratio(bad, r["W"], r["W_bound"]) > FACTOR and R.tile_ratio(bad, r["W"], r["W_bound"], ct=cw) > FACTOR


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if R.facts(c)["nct"] >= 2][::3])
def test_a_missing_q_partial(name, refs):
    r = refs(name)
    c, f = r["case"], R.facts(r["case"])
    Ws = np.asarray(r["W"], np.float64)
    q, qb, q2, qb2 = R.q_ref(c, Ws, r["W"], r["W_bound"])
    for ct in (0, f["nct"] - 1):
        part = (Ws[:, ct * f["cw"]:(ct + 1) * f["cw"]] ** 2).sum(1)
        assert R.ratio(q - part, q, qb) > FACTOR and R.ratio(q2 - part, q2, qb2) > FACTOR, (name, ct)


@pytest.mark.parametrize("name", _claiming("root"))
def test_r2_without_the_1e_12_under_the_root(name, refs):
    r = refs(name)
    c, st = r["case"], r["st"]
    bad = R.knm(c, st["X"], st["Z"], st["params"], root_eps=False)["k"]
    e = R.ratio(bad, r["kn"]["k"], r["kn"]["bound"])
    print(name, "%.2e" % e)
    assert e > FACTOR


@pytest.mark.parametrize("name", _claiming("ard"))
def test_an_ard_axis_scaled_twice(name, refs):
    r = refs(name)
    c, st = r["case"], r["st"]
    for axis in range(c["D"]):
        bad = R.knm(c, st["X"], st["Z"], st["params"], twice=axis)["k"]
        assert R.ratio(bad, r["kn"]["k"], r["kn"]["bound"]) > FACTOR, (name, axis)


def test_exact_results_pass_every_measure(refs):
    r = refs("f64_rq_M250_n1025_D2")
    assert R.ratio(r["W"], r["W"], r["W_bound"]) == 0 and R.tile_ratio(r["W"], r["W"], r["W_bound"]) == 0
    val, bnd = r["sums"]
    assert all(R.ratio(val[k], val[k], bnd[k]) == 0 for k in val)
