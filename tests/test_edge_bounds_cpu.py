"""CPU: the per-element bound of the edge family (tests/_edge_ref.py) on what a machine
without a GPU can run.

(a) test_oracle_and_cpu_twins: the oracle's sequential fp32 chain (orc.row_sum, orc.sddmm,
    orc.softmax_fwd / bwd, orc.gat_fwd / bwd, the pass-by-pass orc.GatRefLayer) and the CPU
    backend's twins of the HIP kernels (gala_cpu_*, through _abi.call_cpu) against the float64
    reference through assert_bounded, on the graphs and inputs the GPU file
    (tests/test_gpu_edge_bounds.py) uses.  This run is where the constants C come from: the
    oracle's worst |err| / mass per quantity is _edge_ref.MEASURED, C is 8 x that
    (test_c_is_eight_times_the_measured_worst), and every case asserts that the oracle stays
    within 2 x MEASURED, i.e. a quarter of the bound.
(b) test_mutations_*: the checker itself.  The float64 result rounded to fp32, with one of
    five faults of a chunked kernel applied, must be rejected -- while the suite's former
    criterion |err| <= 1e-4 + 1e-4 |ref| accepts the first three on the 2 600-edge row.

Inputs (_edge_ref.edge_inputs): the ranges the suite uses everywhere (logits in [-3, 3], aL,
aR, X, dY, d alpha in [-1, 1]); the spotlight set lifts the logit of the edges at positions 0,
deg - 1, kC - 1 and kC of every row longer than 64 edges to s = +9 (softmax) / aR[col] = +8
(GAT), so each of them carries at least SPOT_WEIGHT / (number of them in the row) of the row's
weight: from 80 x the bound's c with 512-edge chunks down to 3.8 x with 16-edge chunks
(_edge_ref.spot_check, asserted on the float64 reference), where the plain inputs' lightest
edge of a 2 600-edge row is below c.  alpha has one c per input set (_edge_ref.c_alpha).
GALA_TEST_RECORD=<path> appends every check's worst ratios (profiles/edge_bounds_cpu.jsonl).
"""
import numpy as np
import pytest

import _edge_ref as er
import oracle as orc
from _edge_ref import C, FIXED, MEASURED, REF, SLOPE, assert_bounded, c_alpha, edge_inputs, spot_check
from _graphs import check_long_rows_graph, edge_bound_graph as graph, long_rows_graph, to_oracle
from gala import _abi
from test_cpu_backend import HostCsr, P

SHAPES = [(1, 32), (8, 256), (3, 96), (1, 47)]


def test_long_rows_graph_is_what_the_tests_rely_on():
    check_long_rows_graph(long_rows_graph())
    t = graph("long_tiled")
    R, Rt = er.Rows(graph("long")), er.Rows(t)
    assert t.n_seg == 3 and np.array_equal(R.deg, Rt.deg)
    # a tiled row's edges, segment after segment, are the CSR row in order (columns ascending)
    assert np.array_equal(t.col[Rt.order], graph("long").col)


def test_c_is_eight_times_the_measured_worst():
    for k, w in MEASURED.items():
        assert C[k] == er.c_from(w) and 8 * w <= C[k] < 16 * w, k
    assert C == {"alpha": 2e-5, "alpha_spot": 2e-4, "Y": 3e-5, "ds": 1e-5, "daL": 2e-6, "sddmm": 3e-6, "row_sum": 2e-5}


CASES = ([("long", h, F, m, sp) for (h, F) in SHAPES for m in (REF, FIXED) for sp in (None, 512, 16)]
         + [("long_tiled", h, F, m, sp) for (h, F) in SHAPES[:2] for m in (REF, FIXED) for sp in (None, 512)]
         + [(gn, h, F, m, None) for gn in ("empty", "empty_tiled") for (h, F) in ((1, 47), (8, 256)) for m in (REF, FIXED)])


class Worst(dict):
    """Worst oracle |err| / mass per quantity over the cases run so far (python -m pytest -s
    tests/test_edge_bounds_cpu.py prints it at the end: the MEASURED table)."""

    cases = 0

    def take(self, q, v):
        self[q] = max(self.get(q, 0.0), v)


WORST = Worst()


def both(tag, q, oracle, twin, ref, mass, R, per):
    """The oracle's and the CPU twin's result through the same reference and checker; the
    oracle also within 2 x MEASURED (a quarter of the bound; not recorded: the same error)."""
    if oracle is not None:
        WORST.take(q, assert_bounded(f"oracle_{tag}", oracle, ref, mass, C[q], g=R, per=per))
        assert_bounded(f"oracle_quarter_{tag}", oracle, ref, mass, 2 * MEASURED[q], g=R, per=per, record=False)
    if twin is not None:
        assert_bounded(f"cpu_{tag}", twin, ref, mass, C[q], g=R, per=per)


@pytest.mark.parametrize("gname,heads,F,mode,spot", CASES)
def test_oracle_and_cpu_twins(gname, heads, F, mode, spot):
    g = graph(gname)
    i = edge_inputs(g, heads, F, spot)
    R, og, A = i.R, to_oracle(g), HostCsr(g)
    n, H = g.n_rows, heads
    tag = f"{gname}_h{heads}_F{F}_m{mode}_s{spot}"
    qa = "alpha_spot" if spot else "alpha"
    WORST.cases += 1
    f32 = lambda *shape: np.empty(shape, np.float32)  # noqa: E731

    for v, name in ((i.v_pos, "pos"), (i.v_signed, "signed")):
        out = f32(n * H)
        _abi.call_cpu("gala_row_sum_f32", A.ref, P(v), H, 1e-12, P(out), 0, None)
        both(f"row_sum_{name}_{tag}", "row_sum", orc.row_sum(og, v, heads=H, eps=1e-12), out,
             *er.row_sum(R, v, H), R, "row")

    out = f32(R.nnz * H)
    _abi.call_cpu("gala_sddmm_dot_f32", A.ref, P(i.dY), F, P(i.X), F, F, H, P(out), None)
    both(f"sddmm_{tag}", "sddmm", orc.sddmm(og, i.dY, i.X, heads=H), out, *er.sddmm(R, i.dY, i.X, H), R, "edge")

    a_ref, a_mass = er.softmax_fwd(R, i.s, H, mode)
    if spot:
        spot_check(i, a_ref, gat=False)
    out = f32(R.nnz * H)
    _abi.call_cpu("gala_edge_softmax_fwd_f32", A.ref, P(i.s), H, mode, P(out), None)
    both(f"softmax_fwd_{tag}", qa, orc.softmax_fwd(og, i.s, heads=H, mode=mode), out, a_ref, a_mass, R, "edge")
    a32 = a_ref.astype(np.float32)
    _abi.call_cpu("gala_edge_softmax_bwd_f32", A.ref, P(a32), P(i.d), H, mode, P(out), None)
    both(f"softmax_bwd_{tag}", "ds", orc.softmax_bwd(og, a32, i.d, heads=H, mode=mode), out,
         *er.softmax_bwd(R, a32, i.d, H, mode), R, "edge")

    square = g.n_rows == g.n_cols
    fw = er.gat_fwd(R, i.aL, i.aR, i.X, H, SLOPE, mode, stats=True)
    if spot:
        spot_check(i, fw.alpha, gat=True)
    Y_o, al_o = orc.gat_fwd(og, i.aL, i.aR, i.X, heads=H, slope=SLOPE, mode=mode)
    Y, al = f32(n, F), f32(R.nnz * H)
    _abi.call_cpu("gala_gat_fwd_f32", A.ref, P(i.aL), P(i.aR), P(i.X), F, F, H, SLOPE, mode, P(Y), F, P(al), None)
    both(f"gat_alpha_{tag}", qa, al_o, al, fw.alpha, fw.alpha, R, "edge")
    both(f"gat_Y_{tag}", "Y", Y_o, Y, fw.Y, fw.Y_mass, R, "row")

    al32 = fw.alpha.astype(np.float32)
    bw = er.gat_bwd(R, i.aL, i.aR, i.X, i.dY, al32, H, SLOPE, mode)
    dz_o, daL_o = orc.gat_bwd(og, i.aL, i.aR, i.X, i.dY, al32.ravel(), heads=H, slope=SLOPE, mode=mode)
    dz, daL = f32(R.nnz * H), f32(n * H)
    _abi.call_cpu("gala_gat_bwd_f32", A.ref, P(i.aL), P(i.aR), P(i.X), F, P(i.dY), F, F, H, SLOPE, mode, P(al32),
                  P(dz), P(daL), None)
    both(f"gat_daL_{tag}", "daL", daL_o, daL, bw.daL, bw.daL_mass, R, "row")
    both(f"gat_dz_{tag}", "ds", dz_o, dz if mode == FIXED else None, bw.dz, bw.dz_mass, R, "edge")

    if mode != REF or not square:
        return
    # the statistics pair (REF, square): the twin's Y, q, Ym, sma and dX, d_aL; the oracle's
    # pass-by-pass layer (one segment) gives q, Y, dX and a d_aL on its own alpha
    bx = er.gat_bwd(R, i.aL, i.aR, i.X, i.dY, fw.alpha, H, SLOPE, REF, dX=True)
    Y, Ym, q, sma = f32(n, F), f32(n, F), f32(n * H), f32(n * H)
    _abi.call_cpu("gala_gat_fwd_stats_f32", A.ref, P(i.aL), P(i.aR), None, None, P(i.X), F, F, H, SLOPE, P(Y), F,
                  P(q), P(Ym), F, P(sma), None, None, None)
    dX, daL = f32(n, F), f32(n * H)
    _abi.call_cpu("gala_gat_bwd_stats_f32", A.ref, P(i.aL), P(i.aR), None, P(i.dY), F, F, H, SLOPE, P(q), P(Y), F,
                  P(Ym), F, P(sma), P(dX), F, P(daL), None)
    lay = None
    if g.n_seg == 1:
        lay = orc.GatRefLayer(g.rowptr, g.col, n, i.X, i.dY, i.aL, i.wR, i.bR, H, slope=SLOPE,
                              row_ids=np.arange(n), aR=i.aR).run()
    L = lambda k: None if lay is None else getattr(lay, k)  # noqa: E731
    both(f"stats_Y_{tag}", "Y", L("Y"), Y, fw.Y, fw.Y_mass, R, "row")
    both(f"stats_q_{tag}", qa, L("q"), q, fw.q, fw.q, R, "row")
    both(f"stats_Ym_{tag}", "Y", None, Ym, fw.Ym, fw.Ym_mass, R, "row")
    both(f"stats_sma_{tag}", "Y", None, sma, fw.sma, fw.sma, R, "row")
    both(f"stats_dX_{tag}", "Y", L("dX"), dX, bx.dX, bx.dX_mass, R, "row")
    both(f"stats_daL_{tag}", "daL", L("daL"), daL, bx.daL, bx.daL_mass, R, "row")


def test_measured_is_the_oracles_worst():
    """MEASURED from the other side: when every case above ran in this process (the file run
    whole, in order), the worst the oracle reached is within 5 % of each recorded value -- a
    MEASURED that has gone stale and too large, i.e. a loose C, fails here.  (Each case already
    asserts oracle <= 2 x MEASURED.)  With a subset of the cases there is nothing to compare."""
    print("\nworst oracle |err| / mass:", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})
    if WORST.cases < len(CASES):
        return
    for q, w in MEASURED.items():
        assert w / 1.05 <= WORST[q] <= 2 * w, (q, WORST[q], w)


# ---- (b) the checker against the faults of a chunked kernel --------------------------------
def old_criterion_accepts(got, ref):
    """The suite's former criterion: |err| <= 1e-4 + 1e-4 |ref| everywhere."""
    return bool(np.all(np.abs(np.asarray(got, np.float64) - ref) <= 1e-4 + 1e-4 * np.abs(ref)))


def rejected(name, got, ref, mass, c, R, per):
    with pytest.raises(AssertionError, match="row"):
        assert_bounded(name, got, ref, mass, c, g=R, per=per, chunk=512)
    return True


class Mut:
    """The float64 GAT / softmax results of long_rows_graph() (one head, F = 32), rounded to
    fp32 as a kernel would return them, and the pieces the mutations recombine."""

    def __init__(self, spot, mode=REF, chunk=512):
        self.g, self.Cn, self.mode, self.ca = graph("long"), chunk, mode, c_alpha(spot)
        self.i = i = edge_inputs(self.g, 1, 32, spot)
        self.R = R = i.R
        self.fw = er.gat_fwd(R, i.aL, i.aR, i.X, 1, SLOPE, mode, stats=True)
        self.a32 = self.fw.alpha.astype(np.float32)
        self.bw = er.gat_bwd(R, i.aL, i.aR, i.X, i.dY, self.a32, 1, SLOPE, mode, dX=True)
        self.sm, _ = er.softmax_fwd(R, i.s, 1, mode)
        self.long = np.flatnonzero(R.deg > chunk)             # rows with at least two chunks
        self.f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731

    def edge(self, r, k):
        """Index of the edge at position k of row r (one segment: CSR order)."""
        return int(self.R.start[r] + k)

    def boundary_edge(self, r, alpha):
        """The heavier of the two edges at the first chunk boundary (positions C - 1, C)."""
        a, b = self.edge(r, self.Cn - 1), self.edge(r, self.Cn)
        return a if alpha[a] >= alpha[b] else b


@pytest.fixture(scope="module")
def plain():
    return Mut(None)


@pytest.fixture(scope="module")
def lit():
    return Mut(512)


def all_ok(m):
    """The unmutated fp32 roundings pass (the mutations alone are what is rejected)."""
    R, fw, bw = m.R, m.fw, m.bw
    assert_bounded("alpha", m.f32(fw.alpha), fw.alpha, fw.alpha, m.ca, g=R, per="edge")
    assert_bounded("Y", m.f32(fw.Y), fw.Y, fw.Y_mass, C["Y"], g=R, per="row")
    assert_bounded("dX", m.f32(bw.dX), bw.dX, bw.dX_mass, C["Y"], g=R, per="row")
    assert_bounded("daL", m.f32(bw.daL), bw.daL, bw.daL_mass, C["daL"], g=R, per="row")


@pytest.mark.parametrize("inputs_", ["plain", "lit"])
def test_mutations_1_to_4_are_rejected(inputs_, request):
    """1: alpha of one long row scaled by 1 +- 1e-3.  2: the denominator missing the edge at
    position C - 1 or C (the heavier; on the plain inputs its weight is asserted > 1.5 c -- a
    lighter edge is within the oracle's own error -- on the spotlight inputs every row
    qualifies).  3: Y, dX or d_aL missing that edge.  4: one whole chunk's partial dropped
    from Y, d_aL and the chunked row sum.  Every row with at least two 512-edge chunks."""
    m = request.getfixturevalue(inputs_)
    all_ok(m)
    R, fw, bw, i = m.R, m.fw, m.bw, m.i
    assert sorted(R.deg[m.long]) == [1023, 1024, 1025, 1536, 1537, 2047, 2048, 2049, 2600]
    rs, rs_mass = er.row_sum(R, i.v_signed, 1)
    for r in m.long:
        e0, e1 = int(R.start[r]), int(R.start[r] + R.deg[r])
        row = slice(e0, e1)
        for f in (1 - 1e-3, 1 + 1e-3):                                        # 1
            a = fw.alpha.copy()
            a[row] *= f
            rejected("m1", m.f32(a), fw.alpha, fw.alpha, m.ca, R, "edge")
        e = m.boundary_edge(r, fw.alpha[:, 0])
        w = fw.alpha[e, 0]
        assert w > 1.5 * m.ca, (int(R.deg[r]), w)
        a = fw.alpha.copy()                                                   # 2
        a[row] /= (1 - w)
        rejected("m2", m.f32(a), fw.alpha, fw.alpha, m.ca, R, "edge")
        Y = fw.Y.copy()                                                       # 3
        Y[r] -= w * i.X[R.col[e]]
        rejected("m3_Y", m.f32(Y), fw.Y, fw.Y_mass, C["Y"], R, "row")
        dX = bw.dX.copy()
        dX[r] -= m.a32[e, 0] * i.dY[R.col[e]].astype(np.float64)
        rejected("m3_dX", m.f32(dX), bw.dX, bw.dX_mass, C["Y"], R, "row")
        daL = bw.daL.copy()
        daL[r] -= bw.dz[e]
        rejected("m3_daL", m.f32(daL), bw.daL, bw.daL_mass, C["daL"], R, "row")
        ch = slice(e0 + m.Cn, min(e0 + 2 * m.Cn, e1))                         # 4: the second chunk
        Y = fw.Y.copy()
        Y[r] -= (fw.alpha[ch] * i.X[R.col[ch]]).sum(0)
        rejected("m4_Y", m.f32(Y), fw.Y, fw.Y_mass, C["Y"], R, "row")
        daL = bw.daL.copy()
        daL[r] -= bw.dz[ch].sum(0)
        rejected("m4_daL", m.f32(daL), bw.daL, bw.daL_mass, C["daL"], R, "row")
        v = rs.copy()
        v[r] -= i.v_signed[ch].astype(np.float64).sum()
        rejected("m4_row_sum", m.f32(v), rs, rs_mass, C["row_sum"], R, "row")


def test_the_old_criterion_accepted_mutations_1_to_3_on_the_2600_edge_row(plain):
    """The gap this file closes: on the 2 600-edge row (plain inputs) |err| <= 1e-4 + 1e-4 |ref|
    accepts alpha scaled by 1 +- 1e-3 and a denominator missing an edge, which assert_bounded
    rejects.  A single edge missing from an aggregate it accepts when alpha_e |x| stays under
    1e-4: with the GAT inputs' logits (LeakyReLU of [-2, 2]) the lightest alpha of a 2 600-edge
    row is 1.2e-4, so here that is 3 of the 10 boundary edges for d_aL and none for Y and dX
    (on longer rows, all of them); assert_bounded rejects every one, heavy or light."""
    m = plain
    R, fw, bw, i = m.R, m.fw, m.bw, m.i
    r = int(np.flatnonzero(R.deg == 2600)[0])
    row = slice(int(R.start[r]), int(R.start[r]) + 2600)
    e = m.boundary_edge(r, fw.alpha[:, 0])
    w = fw.alpha[e, 0]
    for f in (1 - 1e-3, 1 + 1e-3, 1 / (1 - w)):
        a = fw.alpha.copy()
        a[row] *= f
        assert old_criterion_accepts(m.f32(a), fw.alpha)
        assert rejected("old_alpha", m.f32(a), fw.alpha, fw.alpha, m.ca, R, "edge")
    # 3: one edge at a chunk boundary (positions kC - 1, kC: ten edges of this row) missing from Y,
    # dX or d_aL.  The old criterion accepts the light ones (alpha_e |x| under 1e-4); the bound
    # rejects every one of those.
    edges = [m.edge(r, k) for b in range(m.Cn, 2600, m.Cn) for k in (b - 1, b)]
    terms = {"Y": (fw.Y, fw.Y_mass, C["Y"], lambda e: fw.alpha[e, 0] * i.X[R.col[e]].astype(np.float64)),
             "dX": (bw.dX, bw.dX_mass, C["Y"], lambda e: m.a32[e, 0] * i.dY[R.col[e]].astype(np.float64)),
             "daL": (bw.daL, bw.daL_mass, C["daL"], lambda e: bw.dz[e])}
    accepted = dict.fromkeys(terms, 0)
    for name, (ref, mass, c, term) in terms.items():
        for e in edges:
            got = ref.copy()
            got[r] -= term(e)
            accepted[name] += old_criterion_accepts(m.f32(got), ref)
            assert rejected(f"old_{name}", m.f32(got), ref, mass, c, R, "row")     # heavy or light
    assert accepted == {"Y": 0, "dX": 0, "daL": 3}, accepted


@pytest.mark.parametrize("lifted", [False, True])
def test_mutation_5_online_softmax_merge_without_the_rescale(lifted):
    """FIXED mode: chunk k holds (m_k, s_k = sum exp(z - m_k)); the merge is S = sum_k s_k
    exp(m_k - M).  With the rescale omitted (S = sum_k s_k) every alpha of a row whose chunks
    have different maxima is off by S_bad / S - 1.  Plain inputs: the maxima of 512 draws differ
    by ~1e-3, and every row where that moves S by more than 1.5 c is rejected (there are some);
    lifted: the logit of each long row's first edge at +9, so chunk 0's maximum is ~6 above the
    others', and every row is rejected."""
    m = Mut(None, mode=FIXED)
    R, i = m.R, m.i
    z_gat, _ = er.logits(R, i.aL, i.aR, 1, SLOPE)
    z_sm = i.s.astype(np.float64)
    if lifted:
        z_sm[R.start[m.long]] = 9.0
    sets = [("softmax", z_sm, er.softmax_fwd(R, z_sm, 1, FIXED)[0].reshape(-1, 1))]
    if not lifted:
        sets.append(("gat", z_gat, m.fw.alpha))
    n_rejected = 0
    for name, z, ref in sets:
        assert_bounded(f"m5_{name}_unmutated", m.f32(ref), ref, ref, C["alpha"], g=R, per="edge")
        for r in m.long:
            e0, e1 = int(R.start[r]), int(R.start[r] + R.deg[r])
            zr = z[e0:e1, 0]
            cuts = list(range(0, e1 - e0, m.Cn)) + [e1 - e0]
            mk = [zr[a:b].max() for a, b in zip(cuts[:-1], cuts[1:])]
            sk = [np.exp(zr[a:b] - mx).sum() for a, b, mx in zip(cuts[:-1], cuts[1:], mk)]
            M = max(mk)
            S, S_bad = sum(s_ * np.exp(x - M) for s_, x in zip(sk, mk)), sum(sk)
            assert max(mk) > min(mk)                           # chunks with different maxima
            if lifted:
                assert S_bad / S - 1 > 0.05
            elif S_bad / S - 1 <= 1.5 * C["alpha"]:
                continue
            a = ref.copy()
            a[e0:e1, 0] = np.exp(zr - M) / S_bad
            n_rejected += rejected(f"m5_{name}", m.f32(a), ref, ref, C["alpha"], R, "edge")
    assert n_rejected >= (len(m.long) if lifted else 1)
