"""TEST INFRASTRUCTURE: the input-space GAT layer over a row partition, run as one process.

The ranks of gala.dist.partition_graph (p2p tables [lower halo | own rows | higher halo]) run
one after another on the rectangular entry points (gala_gat_in_*_rect_f32 / their host twins),
q of the halo rows copied between the ranks' tables by hand with the q pack / unpack calls --
what gala.dist.HaloGatInput does over a communicator.  Shared by tests/test_gat_input_rect_cpu.py
and tests/test_gpu_gat_input_rect.py; the graphs, inputs and tolerances are those of
tests/test_gat_input_cpu.py, tests/test_gat_input_phases_cpu.py and tests/_hub_graphs.py.
"""
from __future__ import annotations

import numpy as np

from gala import _abi
from gala import dist as gdist
from _graphs import PHASE_N, PHASE_STEP
from _hub_graphs import PlannedCsr
from test_cpu_backend import P, HostCsr

# (world, bounds) over the 8205-row fixtures (phase_graph, hub_sym_graph): uneven cuts, a half
# still longer than one phase of the persistent grid (PHASE_STEP rows)
PARTITIONS = (
    (1, (0, PHASE_N)),
    (2, (0, 4103, PHASE_N)),              # 4103 and 4102 rows: both past one phase, no multiple of 8
    (3, (0, 2001, 6204, PHASE_N)),        # the middle rank: halo rows on both sides, 4203 rows
    (3, (0, 4099, 4099, PHASE_N)),        # the middle rank owns no row
)
PARTITION_IDS = ["P1", "P2", "P3-middle", "P3-empty"]


def make_parts(g, bounds):
    b = np.asarray(bounds, np.int64)
    world = len(b) - 1
    return [gdist.partition_graph(g, r, world, bounds=b, halo_mode="p2p") for r in range(world)]


def check_partitions(g):
    """The properties the rectangular tests rely on, over all of PARTITIONS: a rank with halo
    rows on both sides (so row_base > 0), a rank whose row count is no multiple of 8, a rank
    without rows, a rank longer than one phase of the persistent grid at every world size."""
    both = odd = empty = False
    for world, bounds in PARTITIONS:
        parts = make_parts(g, bounds)
        assert len(parts) == world and sum(p.n for p in parts) == g.n_rows
        assert max(p.n for p in parts) > PHASE_STEP
        for p in parts:
            assert p.own_offset() == p.lo and p.graph.n_rows == p.n and p.graph.n_cols == p.n_cols >= p.n
            assert p.n_cols - p.n == p.n_halo_rows == int(p.recv_counts.sum())
            both |= p.lo > 0 and p.lo + p.n < p.n_cols
            odd |= p.n % 8 != 0
            empty |= p.n == 0
            if world == 1:
                assert p.lo == 0 and p.n_cols == g.n_rows
    assert both and odd and empty


def host_csr(hg, plan):
    return HostCsr(hg) if plan is None else PlannedCsr(hg, *plan)


def halo_lists(parts):
    """[(dst rank, src rank, rows of dst's table, rows of src's table)] for every halo block."""
    out = []
    for p in parts:
        gl = p.xs_to_global()
        idx = np.concatenate([np.arange(0, p.lo), np.arange(p.lo + p.n, p.n_cols)]).astype(np.int64)
        owner = np.searchsorted(p.bounds, gl[idx], side="right") - 1
        for o in parts:
            sel = idx[owner == o.rank]
            if sel.size:
                assert o.rank != p.rank
                out.append((p.rank, o.rank, sel.astype(np.int32), (o.lo + gl[sel] - o.r0).astype(np.int32)))
    return out


def cpu_copy_q(parts, xexts, heads):
    """q of every halo row from its owner's table (gala_cpu_gat_in_q_gather_f32) into the reader's
    (gala_cpu_gat_in_q_scatter_f32)."""
    for dst, src, drows, srows in halo_lists(parts):
        buf = np.empty((len(srows), heads), np.float32)
        _abi.call_cpu("gala_gat_in_q_gather_f32", len(srows), P(srows), xexts[src].shape[0], heads, P(xexts[src]),
                      P(buf), None)
        _abi.call_cpu("gala_gat_in_q_scatter_f32", len(drows), P(drows), 0, xexts[dst].shape[0], heads, P(buf),
                      P(xexts[dst]), None)


def cpu_rect_layer(g, bounds, plan, X, W, b, wL, bL, wR, bR, dY, heads, slope=0.2, relu=False):
    """The host twins over the partition `bounds` of g: every rank's prep over its table, the walk
    forward, the q copy, the walk backward over the same local pattern (g symmetric).  Returns the
    concatenated row outputs, the summed partials M, Gw, Gb and the six composed gradients."""
    from test_gat_input_cpu import compose
    parts = make_parts(g, bounds)
    fin, F = X.shape[1], W.shape[0]
    D = F // heads
    u, c = compose(W, b, wL, bL, wR, bR, heads)
    flags = _abi.GALA_GAT_IN_RELU if relu else 0
    xexts, csrs, outs = [], [], []
    for p in parts:
        Xs = np.ascontiguousarray(X[p.xs_to_global()])
        xe = np.zeros((p.n_cols, 128), np.float32)
        _abi.call_cpu("gala_gat_in_prep_f32", p.n_cols, fin, P(Xs), fin, heads, P(u), P(c), P(xe), None)
        A = host_csr(p.graph, plan)
        Y, Ym = np.empty((p.n, F), np.float32), np.empty((p.n, F), np.float32)
        q, sma = np.empty((p.n, heads), np.float32), np.empty((p.n, heads), np.float32)
        _abi.call_cpu("gala_gat_in_fwd_rect_f32", A.ref, p.lo, None, fin, heads, D, slope, P(xe), P(W), fin, P(b),
                      P(Y), P(Ym), F, P(q), P(sma), flags, None)
        xexts.append(xe)
        csrs.append(A)
        outs.append(dict(Y=Y, Ym=Ym, q=q, sma=sma))
    cpu_copy_q(parts, xexts, heads)
    wsb = _abi.cpu_lib().gala_cpu_gat_in_bwd_workspace(heads)
    ws = np.empty(wsb // 4, np.float32)
    Ms, Gws, Gbs = [], [], []
    for p, xe, A, o in zip(parts, xexts, csrs, outs):
        dy = np.ascontiguousarray(dY[p.r0:p.r0 + p.n])
        daL = np.empty((p.n, heads), np.float32)
        M = np.empty((heads, D, fin + 1), np.float32)
        _abi.call_cpu("gala_gat_in_bwd_rect_f32", A.ref, p.lo, None, fin, heads, D, slope, P(xe), P(dy), P(o["Y"]),
                      P(o["Ym"]), F, P(o["sma"]), P(daL), P(M), P(ws), wsb, flags, None)
        o["daL"] = daL
        Xo = np.ascontiguousarray(X[p.r0:p.r0 + p.n])
        Gw, Gb = np.zeros((heads, fin), np.float32), np.zeros(heads, np.float32)
        if p.n:
            gwb = _abi.cpu_lib().gala_cpu_dense_grad_workspace(p.n, fin, heads)
            gws = np.empty(max(gwb // 4, 1), np.float32)
            _abi.call_cpu("gala_dense_grad_f32", p.n, fin, heads, P(Xo), fin, P(daL), heads, P(Gw), P(Gb), 0, P(gws),
                          gwb, None)
        Ms.append(M)
        Gws.append(Gw)
        Gbs.append(Gb)
    res = {k: np.concatenate([o[k] for o in outs]) for k in ("Y", "Ym", "q", "sma", "daL")}
    res.update(compose_grads(sum_parts(Ms), sum_parts(Gws), sum_parts(Gbs), W, b, wL, wR, heads))
    res["M_parts"], res["parts"], res["xexts"] = Ms, parts, xexts
    return res


def sum_parts(arrs):
    """The ranks' partials added in rank order in float32 (what an all-reduce's sum may do)."""
    out = arrs[0].copy()
    for a in arrs[1:]:
        out = out + a
    return out


def compose_grads(M, Gw, Gb, W, b, wL, wR, heads):
    """test_gat_input_cpu.cpu_layer's composition of the six parameter gradients from M and G."""
    F, fin = W.shape
    D = F // heads
    sLR = (wL + wR).reshape(heads, D).astype(np.float64)
    dW = (M[:, :, :fin] + sLR[:, :, None] * Gw[:, None, :]).reshape(F, fin)
    db = (M[:, :, fin] + sLR * Gb[:, None]).reshape(F)
    dw = (W.reshape(heads, D, fin) * Gw[:, None, :]).sum(2) + b.reshape(heads, D) * Gb[:, None]
    return dict(M=M, Gw=Gw, Gb=Gb, dW=dW, db=db, dwL=dw.reshape(-1), dbL=Gb)


def check_grads_against_ref(got, ref, X, heads):
    """The existing files' criteria for the parameter gradients: grad_close (1e-4 of the largest
    entry) and the element-wise c * mass bound with GRAD_C."""
    from test_gat_input_cpu import grad_close
    from test_gat_input_phases_cpu import GRAD_C, grad_close_elementwise, grad_masses
    mass = grad_masses(ref, X, heads)
    for k in ("dW", "db", "dwL", "dbL"):
        grad_close(got[k], ref[k], k)
        grad_close_elementwise(got[k], ref[k], mass[k], GRAD_C, k)
