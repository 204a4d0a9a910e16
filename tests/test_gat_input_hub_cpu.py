"""CPU: the input-space GAT layer (gala_gat_in_*) on graphs whose split plan has hub rows.

A hub row (longer than the plan's threshold) is summed as per-chunk partials combined in
chunk order -- the association of the gfx950 pre-pass k_gat_in_chunks and the persistent
kernels' combine -- by libgala_cpu.so's twins; this checks them against the oracle's
pass-by-pass REF layer (tests/test_gat_input_cpu.py's helpers and tolerances) on
_graphs.long_rows_graph (rows of exactly 63..129 and 1023..2600 edges) under the plans
(threshold 64, chunk 64) and the default (1024, 512), forward and -- on the transposed graph
-- backward, and the entry points' contract for such plans.  tests/test_gpu_gat_input_hub.py
runs the kernels against the same twins.
"""
import numpy as np
import pytest

import oracle as orc  # noqa: F401  (the oracle's path, as the helpers below need it)
from gala import _abi, layout
from _graphs import LONG_TEST, check_long_rows_graph, long_rows_graph
from _hub_graphs import PLANS, PlannedCsr
from test_cpu_backend import P
from test_gat_input_cpu import TOL, compose, grad_close, layer_inputs, ref_on_own_logits

_CACHE = {}


def long_graphs():
    """long_rows_graph (checked) and its transpose, built once."""
    if not _CACHE:
        g = long_rows_graph()
        check_long_rows_graph(g)
        _CACHE["g"], _CACHE["gT"] = g, layout.transpose(g)[0]
    return _CACHE["g"], _CACHE["gT"]


def cpu_layer_plan(g, gT, plan, X, W, b, wL, bL, wR, bR, dY, heads, slope=0.2, relu=False):
    """test_gat_input_cpu.cpu_layer with the plan (threshold, chunk) on g and on gT, the
    transposed pattern the backward walks (None: no plan, hub rows are one chain)."""
    from test_cpu_backend import HostCsr
    n, fin = X.shape
    F = W.shape[0]
    D = F // heads
    u, c = compose(W, b, wL, bL, wR, bR, heads)
    xext = np.zeros((n, 128), np.float32)
    _abi.call_cpu("gala_gat_in_prep_f32", n, fin, P(X), fin, heads, P(u), P(c), P(xext), None)
    A, AT = (HostCsr(g), HostCsr(gT)) if plan is None else (PlannedCsr(g, *plan), PlannedCsr(gT, *plan))
    Y, Ym = np.empty((n, F), np.float32), np.empty((n, F), np.float32)
    q, sma = np.empty((n, heads), np.float32), np.empty((n, heads), np.float32)
    flags = _abi.GALA_GAT_IN_RELU if relu else 0
    _abi.call_cpu("gala_gat_in_fwd_f32", A.ref, None, fin, heads, D, slope, P(xext), P(W), fin, P(b), P(Y), P(Ym), F,
                  P(q), P(sma), flags, None)
    daL = np.empty((n, heads), np.float32)
    M = np.empty((heads, D, fin + 1), np.float32)
    wsb = _abi.cpu_lib().gala_cpu_gat_in_bwd_workspace(heads)
    ws = np.empty(wsb // 4, np.float32)
    _abi.call_cpu("gala_gat_in_bwd_f32", AT.ref, None, fin, heads, D, slope, P(xext), P(dY), P(Y), P(Ym), F, P(sma),
                  P(daL), P(M), P(ws), wsb, flags, None)
    Gw, Gb = np.empty((heads, fin), np.float32), np.empty(heads, np.float32)
    gwb = _abi.cpu_lib().gala_cpu_dense_grad_workspace(n, fin, heads)
    gws = np.empty(max(gwb // 4, 1), np.float32)
    _abi.call_cpu("gala_dense_grad_f32", n, fin, heads, P(X), fin, P(daL), heads, P(Gw), P(Gb), 0, P(gws), gwb, None)
    sLR = (wL + wR).reshape(heads, D).astype(np.float64)
    dW = (M[:, :, :fin] + sLR[:, :, None] * Gw[:, None, :]).reshape(F, fin)
    db = (M[:, :, fin] + sLR * Gb[:, None]).reshape(F)
    dw = (W.reshape(heads, D, fin) * Gw[:, None, :]).sum(2) + b.reshape(heads, D) * Gb[:, None]
    hubs = (A.n_rows_split, AT.n_rows_split) if plan is not None else (0, 0)
    return dict(Y=Y, Ym=Ym, q=q, sma=sma, daL=daL, M=M, dW=dW, db=db, dwL=dw.reshape(-1), dbL=Gb, xext=xext, hubs=hubs)


def check_twin_against_ref(got, ref):
    np.testing.assert_allclose(got["Y"], ref["Y"], **TOL)
    np.testing.assert_allclose(got["q"], ref["q"], rtol=1e-4)
    np.testing.assert_allclose(got["daL"], ref["daL"], **TOL)
    for k in ("dW", "db", "dwL", "dbL"):
        grad_close(got[k], ref[k], k)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("plan", PLANS)
def test_twin_sums_hub_rows_as_chunk_partials(plan, transposed):
    """Forward over the hub rows (long_rows_graph) and, on the transposed graph, backward over
    them, against the oracle; rows at or below the threshold are bit-identical to the run
    without a plan."""
    g, gT = long_graphs()
    if transposed:
        g, gT = gT, g
    fin, heads, D = 37, 4, 16
    inp = layer_inputs(g.n_rows, fin, heads, D, seed=31)
    got = cpu_layer_plan(g, gT, plan, *inp, heads, relu=True)
    want_hubs = 15 if plan[0] == 64 else 7
    assert got["hubs"][1 if transposed else 0] == want_hubs     # the hub path is the one under test
    ref = ref_on_own_logits(g, got, *inp, heads, relu=True)
    check_twin_against_ref(got, ref)
    base = cpu_layer_plan(g, gT, None, *inp, heads, relu=True)
    rows = np.diff(g.rowptr) <= plan[0]
    for k in ("Y", "Ym", "q", "sma"):
        assert np.array_equal(got[k][rows], base[k][rows]), k
    if not transposed:      # the hub rows themselves are regrouped: not the same bits
        assert not np.array_equal(got["Y"][~rows], base["Y"][~rows])


def test_a_lost_last_chunk_fails_the_check():
    """The 129-edge row under (64, 64) ends in a one-edge chunk.  The twin on the graph without
    that edge is what a combine that dropped the last chunk computes: the q comparison above
    must fail on that row (one edge in 129 moves q by far more than rtol 1e-4: the logits are
    bounded) and on no other."""
    g, gT = long_graphs()
    deg = np.diff(g.rowptr)
    row = int(np.flatnonzero(deg == 129)[0])
    assert 129 in LONG_TEST and 129 % 64 == 1
    last = int(g.rowptr[row + 1]) - 1
    src = np.delete(np.repeat(np.arange(g.n_rows, dtype=np.int32), deg), last)
    cut = layout.csr_build(g.n_rows, g.n_cols, src, np.delete(g.col, last))
    assert np.diff(cut.rowptr)[row] == 128 and cut.nnz == g.nnz - 1
    fin, heads, D = 37, 4, 16
    inp = layer_inputs(g.n_rows, fin, heads, D, seed=31)
    got = cpu_layer_plan(cut, layout.transpose(cut)[0], (64, 64), *inp, heads)
    ref = ref_on_own_logits(g, got, *inp, heads)
    others = np.arange(g.n_rows) != row
    np.testing.assert_allclose(got["q"][others], ref["q"][others], rtol=1e-4)
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(got["q"][row], ref["q"][row], rtol=1e-4)
    with pytest.raises(AssertionError):
        check_twin_against_ref(got, ref)


def test_hub_plan_contract():
    g, gT = long_graphs()
    n, fin, heads, D = g.n_rows, 37, 4, 16
    F = heads * D
    xext, W = np.zeros((n, 128), np.float32), np.zeros((F, fin), np.float32)
    Y, q = np.zeros((n, F), np.float32), np.zeros((n, heads), np.float32)
    M, daL = np.zeros((heads, D, fin + 1), np.float32), np.zeros((n, heads), np.float32)
    ws = np.zeros(8, np.float32)

    def fwd(fn, A):
        return fn(A.ref, None, fin, heads, D, 0.2, P(xext), P(W), fin, None, P(Y), P(Y), F, P(q), P(q), 0, None)

    def bwd(fn, A, wsb):
        return fn(A.ref, None, fin, heads, D, 0.2, P(xext), P(Y), P(Y), P(Y), F, P(q), P(daL), P(M), P(ws), wsb, 0, None)

    C, G = _abi.cpu_lib(), _abi.lib()
    # a chunk that is not a whole number of 64-index column windows: unsupported on both backends
    bad = PlannedCsr(g, 64, 32)
    assert bad.n_rows_split == 15
    assert fwd(C.gala_cpu_gat_in_fwd_f32, bad) == _abi.GALA_ERR_UNSUPPORTED
    assert bwd(C.gala_cpu_gat_in_bwd_f32, bad, 1 << 30) == _abi.GALA_ERR_UNSUPPORTED
    assert fwd(G.gala_gat_in_fwd_f32, bad) == _abi.GALA_ERR_UNSUPPORTED
    assert bwd(G.gala_gat_in_bwd_f32, bad, 1 << 30) == _abi.GALA_ERR_UNSUPPORTED
    # the workspace sizes: the forward walk, the forward in T mode, the backward walk
    cols = [G.gala_gat_in_split_ws_cols(m) for m in
            (_abi.GALA_GAT_IN_WS_FWD, _abi.GALA_GAT_IN_WS_FWD_T, _abi.GALA_GAT_IN_WS_BWD)]
    assert cols[0] == 16 * 7 * 16 and cols[2] == 8 * 7 * 16 and cols[1] >= cols[0] + cols[2]
    assert all(c > 0 and c % 4 == 0 for c in cols)
    assert G.gala_gat_in_split_ws_cols(3) == -1 and G.gala_gat_in_split_ws_cols(-1) == -1
    # a valid plan without a workspace (or with a small one): invalid, before any launch
    ok = PlannedCsr(g, 64, 64)
    assert ok.n_rows_split == 15
    assert fwd(G.gala_gat_in_fwd_f32, ok) == _abi.GALA_ERR_INVALID_ARG
    assert bwd(G.gala_gat_in_bwd_f32, ok, 1 << 30) == _abi.GALA_ERR_INVALID_ARG
    small = np.zeros(ok.n_chunks * 64 + 4, np.float32)
    ok.plan.workspace, ok.plan.ws_cols = (small.ctypes.data + 15) // 16 * 16, 64
    assert fwd(G.gala_gat_in_fwd_f32, ok) == _abi.GALA_ERR_INVALID_ARG
