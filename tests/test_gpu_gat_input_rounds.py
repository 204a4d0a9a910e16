"""GPU: the input-space GAT kernels' grid-stride loops past their first round.

k_gat_in_chunks<0, 1, 2> (the hub rows' pre-pass: one wave per chunk, 4096 waves) on
_rounds.round_hub_graph, whose plan (64, 64) has more than 2 * 4096 chunks: while a wave sums
chunk c, cursor_walk requests chunk c + 4096's bounds, window, side values and first batch, and
the last round hands off to nothing.  The checks are tests/test_gpu_gat_input_hub.py's, at its
tolerances: the oracle's REF layer on the kernels' own logits, the host twins (shown good on
these graphs by tests/test_gat_input_rounds_cpu.py), rows at or below the threshold
bit-identical to a run without a plan, T mode bit-identical to the walk, two calls
bit-identical, and the spotlight gradient.

k_gat_in_prep (65 536 rows per round) and k_gat_in_q (262 144) on _rounds.prep_q_graph, called
alone.  k_gat_in_q_chunks, the hub rows' share of the q pass, loops only past 262 144 chunks;
at 2696 floats of workspace per chunk that is several GB and no few-second test, so its second
round stays uncovered (the section on grid caps).
"""
import numpy as np
import pytest
import torch

from gala import _abi, layout, ops
from _hub_graphs import PlannedCsr
from _rounds import (CHUNK_ROUND, PREP_Q_HUBS, PREP_Q_N, PREP_ROUND, Q_ROUND, ROUND_PLAN, check_prep_q_graph,
                     prep_q_graph)
from test_cpu_backend import P
from test_gat_input_cpu import grad_close, layer_inputs, ref_on_own_logits
from test_gat_input_rounds_cpu import SHAPES, n_hub_rows, round_graphs
from test_gpu_gat_input import check_against_ref, dev
from test_gpu_gat_input_hub import gpu_layer, planned

pytestmark = pytest.mark.gpu


def past_one_round(kind):
    g, gT, side = round_graphs(kind)
    A = PlannedCsr(gT if side else g, *ROUND_PLAN)
    nr = A.n_rows_split
    assert A.n_chunks > 2 * CHUNK_ROUND and nr == n_hub_rows(kind)     # three rounds for the first wave slots
    return g, gT, side, nr


def host_layer_on(xext, g, gT, X, W, b, wL, bL, wR, bR, dY, heads, slope=0.2):
    """test_gat_input_hub_cpu.cpu_layer_plan under ROUND_PLAN from the extended rows given (the
    kernels' own, so both sides take the same side of the LeakyReLU kink on every edge) instead
    of the host's gala_gat_in_prep_f32."""
    n, fin = X.shape
    F = W.shape[0]
    D = F // heads
    xext = xext.copy()
    A, AT = PlannedCsr(g, *ROUND_PLAN), PlannedCsr(gT, *ROUND_PLAN)
    Y, Ym = np.empty((n, F), np.float32), np.empty((n, F), np.float32)
    q, sma = np.empty((n, heads), np.float32), np.empty((n, heads), np.float32)
    _abi.call_cpu("gala_gat_in_fwd_f32", A.ref, None, fin, heads, D, slope, P(xext), P(W), fin, P(b), P(Y), P(Ym), F,
                  P(q), P(sma), 0, None)
    daL = np.empty((n, heads), np.float32)
    M = np.empty((heads, D, fin + 1), np.float32)
    wsb = _abi.cpu_lib().gala_cpu_gat_in_bwd_workspace(heads)
    ws = np.empty(wsb // 4, np.float32)
    _abi.call_cpu("gala_gat_in_bwd_f32", AT.ref, None, fin, heads, D, slope, P(xext), P(dY), P(Y), P(Ym), F, P(sma),
                  P(daL), P(M), P(ws), wsb, 0, None)
    Gw, Gb = np.empty((heads, fin), np.float32), np.empty(heads, np.float32)
    gwb = _abi.cpu_lib().gala_cpu_dense_grad_workspace(n, fin, heads)
    gws = np.empty(max(gwb // 4, 1), np.float32)
    _abi.call_cpu("gala_dense_grad_f32", n, fin, heads, P(X), fin, P(daL), heads, P(Gw), P(Gb), 0, P(gws), gwb, None)
    sLR = (wL + wR).reshape(heads, D).astype(np.float64)
    dW = (M[:, :, :fin] + sLR[:, :, None] * Gw[:, None, :]).reshape(F, fin)
    return dict(Y=Y, daL=daL, dW=dW)


def against_host_twins(g, gT, inp, heads, tmode=False):
    """The kernels against libgala_cpu.so's twins under the plan, at tests/test_gpu_gat_input_hub.py's
    tolerances (the same sums in the same order, exp aside).  Two things keep a discontinuity
    out of the comparison, which among these graphs' 4.4 M outputs and 4.3 M (edge, head) logits
    is otherwise hit (seen on the directed graphs: one d_aL entry off by 0.03, the fin entries
    of one dW row).  The twins start from the kernels' own extended rows: the host composes u
    and c with other roundings, and a logit within an ulp of 0 then takes the other LeakyReLU
    slope there, which moves sma and d_aL of its row by a whole alpha (DESIGN.md section 3;
    gala_gat_in_prep_f32 itself is compared bit for bit below).  And no fused ReLU: each side
    masks dY by its own Y > 0; the fused ReLU is checked against the oracle on the kernels'
    own mask."""
    got = gpu_layer(g, *inp, heads, gT=gT, tmode=tmode, plan=ROUND_PLAN)
    host = host_layer_on(got["xext"], g, g if gT is None else gT, *inp, heads)
    np.testing.assert_allclose(got["Y"], host["Y"], atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(got["daL"], host["daL"], atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(got["dW"], host["dW"], atol=1e-5 * np.abs(host["dW"]).max())


@pytest.mark.parametrize("kind", ["dir", "dirT"])
@pytest.mark.parametrize("fin,heads,D", SHAPES)
def test_walk_over_chunks_past_one_round(fin, heads, D, kind):
    """dir: the forward's pre-pass (MODE 0) over the checked graph's chunks; dirT: the layer on
    its transpose, whose backward's pre-pass (MODE 2) walks them."""
    g, gT, side, nr = past_one_round(kind)
    inp = layer_inputs(g.n_rows, fin, heads, D, seed=fin + heads)
    got = gpu_layer(g, *inp, heads, gT=gT, relu=True, plan=ROUND_PLAN)
    assert got["hubs"][side] == nr
    check_against_ref(got, ref_on_own_logits(g, got, *inp, heads, relu=True))
    against_host_twins(g, gT, inp, heads)
    base = gpu_layer(g, *inp, heads, gT=gT, relu=True)
    rows = np.diff(g.rowptr) <= ROUND_PLAN[0]
    for k in ("Y", "Ym", "q", "sma"):
        assert np.array_equal(got[k][rows], base[k][rows]), k


@pytest.mark.parametrize("fin,heads,D", SHAPES)
def test_symmetric_walk_and_t_mode_past_one_round(fin, heads, D):
    """The walk (MODE 0 forward, MODE 2 backward) and T mode (MODE 1) on the symmetric graph:
    each against the oracle and the host twins, T mode bit-identical to the walk on every
    output."""
    g, _, _, nr = past_one_round("sym")
    inp = layer_inputs(g.n_rows, fin, heads, D, seed=41)
    runs = {}
    for tm in (False, True):
        got = gpu_layer(g, *inp, heads, relu=True, tmode=tm, plan=ROUND_PLAN)
        assert got["hubs"][0] == nr
        check_against_ref(got, ref_on_own_logits(g, got, *inp, heads, relu=True))
        runs[tm] = got
    against_host_twins(g, None, inp, heads, tmode=True)
    for k in ("Y", "Ym", "q", "sma", "daL", "M", "dW", "db", "dwL", "dbL"):
        assert np.array_equal(runs[False][k], runs[True][k]), k


@pytest.mark.parametrize("tmode", [False, True])
def test_spotlight_gradient_past_one_round(tmode):
    """dY zero except on the hub rows: M and dW are the hub columns' aggregates alone, so a lost
    chunk of any round cannot hide under 1e-4 of another column's entries."""
    g, _, _, _ = past_one_round("sym")
    fin, heads, D = 100, 8, 32
    X, W, b, wL, bL, wR, bR, dY = layer_inputs(g.n_rows, fin, heads, D, seed=43)
    dY[np.diff(g.rowptr) <= ROUND_PLAN[0]] = 0
    got = gpu_layer(g, X, W, b, wL, bL, wR, bR, dY, heads, tmode=tmode, plan=ROUND_PLAN)
    ref = ref_on_own_logits(g, got, X, W, b, wL, bL, wR, bR, dY, heads)
    check_against_ref(got, ref)
    for k in ("dW", "db"):
        grad_close(got[k], ref[k], k)


@pytest.mark.parametrize("tmode", [False, True])
def test_two_calls_past_one_round_are_bit_identical(tmode):
    g, _, _, _ = past_one_round("sym")
    inp = layer_inputs(g.n_rows, 100, 8, 32, seed=53)
    a = gpu_layer(g, *inp, 8, relu=True, tmode=tmode, plan=ROUND_PLAN)
    b = gpu_layer(g, *inp, 8, relu=True, tmode=tmode, plan=ROUND_PLAN)
    for k in ("Y", "Ym", "q", "sma", "daL", "M") + (("T",) if tmode else ()):
        assert np.array_equal(a[k], b[k]), k


# ---- k_gat_in_prep and k_gat_in_q, called alone -----------------------------------------------
Q_SLOTS = [116 + 4 * (h // 3) + h % 3 for h in range(8)]     # gat_input.hip q_slot(h)
AL_SLOTS = [99 + 4 * h for h in range(8)]                    # aL_slot(h)
AR_SLOTS = [67 + 4 * h for h in range(8)]                    # aR_slot(h)
_PQ = {}


def prep_q_inputs():
    if not _PQ:
        g = prep_q_graph()
        check_prep_q_graph(g)
        rng = np.random.default_rng(5)
        _PQ.update(g=g, X=rng.uniform(-1, 1, (g.n_rows, 100)).astype(np.float32))
    return _PQ["g"], _PQ["X"]


def host_q(g, xext, heads):
    """q of the host twin's forward under the plan (D = 4, W = 0: only q is read): the row's p
    summed in CSR order, a hub row's as per-chunk sums added in chunk order -- the association
    of k_gat_in_q and of k_gat_in_q_chunks / k_gat_in_q_hub."""
    n, F = g.n_rows, 4 * heads
    A = PlannedCsr(g, *ROUND_PLAN)
    assert A.n_rows_split == len(PREP_Q_HUBS)
    W = np.zeros((F, 100), np.float32)
    Y, Ym = np.empty((n, F), np.float32), np.empty((n, F), np.float32)
    q, sma = np.empty((n, heads), np.float32), np.empty((n, heads), np.float32)
    table = xext.copy()          # (the forward writes q into it)
    _abi.call_cpu("gala_gat_in_fwd_f32", A.ref, None, 100, heads, 4, 0.2, P(table), P(W), 100, None, P(Y), P(Ym),
                  F, P(q), P(sma), 0, None)
    return q


def q_float64(g, xext, heads):
    """1 / (1e-12 + sum_e p) per row and head in float64, from the table's own float32 logits
    with the kernel's per-edge roundings (t = fl(aL + aR), the LeakyReLU product in float32)."""
    deg = np.diff(g.rowptr.astype(np.int64))
    row = np.repeat(np.arange(g.n_rows), deg)
    out = np.empty((g.n_rows, heads))
    for h in range(heads):
        t = xext[row, AL_SLOTS[h]] + xext[g.col, AR_SLOTS[h]]
        z = np.where(t > 0, t, t * np.float32(0.2)).astype(np.float32)
        p = np.minimum(np.exp(z.astype(np.float64)), 1e12)
        out[:, h] = 1.0 / (np.bincount(row, weights=p, minlength=g.n_rows) + np.float64(np.float32(1e-12)))
    return out


@pytest.mark.parametrize("heads", [8, 3])
def test_prep_and_q_past_one_round(heads):
    """gala_gat_in_prep_f32 (five rounds) and the q pass gala_gat_in_q_rect_f32 (two rounds of
    k_gat_in_q; the `continue` of a lane with h >= H and of a hub row taken in both) alone, on
    262 221 rows.  The extended rows: bit for bit the host twin's (no exp in them), the logits
    within 1e-5 of float64 (test_gat_input_cpu.ref_on_own_logits' bound).  q: every slot the
    pass owns is written (a NaN sentinel first) and no other; bit for bit the q of
    single-round launches of the same kernels over three row slices (the rect entry point,
    row_base = the slice's first row); within 2e-6 of the host twin's (the twins' tolerance in
    tests/test_gpu_gat_input_hub.py: the same sums in the same order, the host's expf aside --
    the count of q that differ in their bits is printed) and rtol 1e-4 of float64
    (tests/test_gpu_gat_input.py's tolerance for q)."""
    g, X = prep_q_inputs()
    n, fin = g.n_rows, 100
    assert n == PREP_Q_N and n > 4 * PREP_ROUND and n > Q_ROUND
    rng = np.random.default_rng(heads)
    u = (rng.uniform(-1, 1, (2 * heads, fin)) / np.sqrt(fin)).astype(np.float32)
    c = rng.uniform(-0.1, 0.1, 2 * heads).astype(np.float32)
    xext = torch.full((n, 128), float("nan"), device="cuda")
    ops.gat_in_prep(dev(X), dev(u), dev(c), heads, xext=xext)
    torch.cuda.synchronize()
    xe = xext.cpu().numpy()
    for lo, hi in ((0, PREP_ROUND), (PREP_ROUND, Q_ROUND), (Q_ROUND, n)):
        assert np.isfinite(xe[lo:hi]).all(), (lo, hi)      # every slot of every row, every round
    xh = np.zeros((n, 128), np.float32)
    _abi.call_cpu("gala_gat_in_prep_f32", n, fin, P(X), fin, heads, P(u), P(c), P(xh), None)
    bad = np.flatnonzero((xe.view(np.uint32) != xh.view(np.uint32)).any(1))
    assert bad.size == 0, f"{bad.size} extended rows differ from the host twin's, the first row {bad[0]}"
    X64 = X.astype(np.float64)
    lg = X64 @ u.astype(np.float64).T + c
    np.testing.assert_allclose(xe[:, AL_SLOTS[:heads]], lg[:, :heads], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(xe[:, AR_SLOTS[:heads]], lg[:, heads:], atol=1e-5, rtol=1e-5)

    # the q pass: NaN in the slots it owns, a sentinel in the q slots of the heads past H
    xext[:, Q_SLOTS[:heads]] = float("nan")
    xext[:, Q_SLOTS[heads:]] = 7.0
    before = xext.clone()
    dg = planned(g, ROUND_PLAN)
    assert dg.split_rows == len(PREP_Q_HUBS)
    ops.gat_in_q(dg, xext, heads)
    torch.cuda.synchronize()
    own = torch.zeros(128, dtype=torch.bool, device="cuda")
    own[Q_SLOTS[:heads]] = True
    assert torch.equal(xext[:, ~own], before[:, ~own])                 # nothing else is written
    q = xext[:, Q_SLOTS[:heads]].cpu().numpy()
    for lo, hi in ((0, PREP_ROUND), (PREP_ROUND, Q_ROUND), (Q_ROUND, n)):
        assert np.isfinite(q[lo:hi]).all(), (lo, hi, int(np.flatnonzero(~np.isfinite(q[lo:hi]).all(1))[0]) + lo)
    # single-round launches over row slices, bit for bit
    deg = np.diff(g.rowptr)
    cuts = [0, 65_000, 200_001, n]                             # a hub row in every slice
    assert max(b - a for a, b in zip(cuts, cuts[1:])) <= Q_ROUND
    for lo, hi in zip(cuts, cuts[1:]):
        rp = (g.rowptr[lo:hi + 1] - g.rowptr[lo]).astype(np.int32)
        sub = layout.HostGraph(hi - lo, n, rp, g.col[g.rowptr[lo]:g.rowptr[hi]].copy(), None)
        ds = planned(sub, ROUND_PLAN)
        assert ds.split_rows == int((deg[lo:hi] > ROUND_PLAN[0]).sum()) >= 1
        xs = before.clone()
        ops.gat_in_q(ds, xs, heads, row_base=lo)
        torch.cuda.synchronize()
        assert torch.equal(xs[lo:hi], xext[lo:hi]), (lo, hi)
    hq = host_q(g, xe, heads)
    print(f"q, heads {heads}: {int((q.view(np.uint32) != hq.view(np.uint32)).sum())} of {q.size} differ in their "
          f"bits from the host twin's, worst relative difference {float(np.max(np.abs(q - hq) / hq)):.3g}")
    np.testing.assert_allclose(q, hq, atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(q, q_float64(g, xe, heads), rtol=1e-4)
    assert np.all(q[deg == 0] == np.float32(1e12))
