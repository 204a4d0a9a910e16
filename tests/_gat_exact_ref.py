"""TEST INFRASTRUCTURE: float64 reference of the exact GAT pair (gala_gat_{fwd,bwd}_stats_exact_f32:
the stable softmax and its true gradients on a symmetric pattern), with the mass of every
element, the graphs and inputs of its tests, and the constants of its bounds.

Per head, t = fl32(aL[r] + aR[c]) (the fp32 logit, formed as the kernels form it, so every
edge's LeakyReLU branch is the kernels'), s = m t with m = 1 where t > 0, else slope:

    forward   alpha_rc = exp(s - lse_r), lse_r = max_c s + log sum_c exp(s - max)
              Y = sum_c alpha X[c], Ym = sum_c m alpha X[c], sma = sum_c m alpha
    backward  g[r] = <dY[r], Y[r]>_h,  d_aL[r] = <dY[r], Ym[r]>_h - g[r] sma[r]
              dX[c] = sum_r alpha_rc dY[r],  dXm[c] = sum_r m alpha_rc dY[r],
              sg[c] = sum_r m alpha_rc g[r],  d_aR[c] = <dXm[c], X[c]>_h - sg[c]

the backward's sums over row c's stored neighbours r (the in-edges (r, c) of a symmetric
pattern).  tests/test_gat_exact_cpu.py::test_reference_is_the_derivative checks these formulas
against torch.autograd of the dense float64 layer.

Bounds: |got - ref| <= c * mass + 1e-12 on every element (_edge_ref.assert_bounded), mass the
float64 sum of the absolute values of every term that enters the element; lse = max + log(sum)
has mass |max| + |log sum| + 1 (a relative error of the sum is an absolute one of its log).
c per quantity is 8 x the host twins' worst |twin - float64| / mass over CASES, rounded up to
one significant digit (_edge_ref.c_from), measured by
tests/test_gat_exact_cpu.py::test_twins_against_float64 (profiles/gat_exact_bounds_cpu.jsonl):

    quantity      worst twin err / mass      c
    Y, Ym         8.22e-7                    7e-6
    sma           1.12e-6                    9e-6
    lse           1.58e-7                    2e-6
    dX            3.74e-6                    3e-5
    d_aL          1.42e-7                    2e-6
    d_aR          2.60e-6                    3e-5

dX and d_aR are largest on the inputs with logits past 30: alpha = exp(s - lse) carries the
rounding of s and lse, about 40 * 2^-24 each, where the plain inputs' are about 3 * 2^-24.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import _edge_ref as E
import _graphs as G
import _hub_graphs as HG
from gala import layout

SLOPE = 0.2
QUANTITIES = ("Y", "Ym", "sma", "lse", "dX", "daL", "daR")
# worst |host twin - float64| / mass over CASES (test_twins_against_float64), and c = 8 x that
MEASURED = {"Y": 8.22e-7, "Ym": 8.22e-7, "sma": 1.12e-6, "lse": 1.58e-7, "dX": 3.74e-6, "daL": 1.42e-7, "daR": 2.60e-6}
C = {k: E.c_from(v) for k, v in MEASURED.items()}
C_AR = E.C["sddmm"]          # the recomputed source logit is one dot per (row, head)


def symmetrise(g: layout.HostGraph, loops=True) -> layout.HostGraph:
    """pattern(g) | pattern(g)^T (| the diagonal with loops), every edge stored once, rows
    sorted by column: a CSR that equals its transpose's."""
    assert g.n_rows == g.n_cols and g.n_seg == 1
    n = g.n_rows
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.rowptr.astype(np.int64)))
    dst = g.col.astype(np.int64)
    u, v = np.concatenate([src, dst]), np.concatenate([dst, src])
    if loops:
        u, v = np.concatenate([u, np.arange(n)]), np.concatenate([v, np.arange(n)])
    key = np.unique(u * n + v)
    s = layout.csr_build(n, n, (key // n).astype(np.int32), (key % n).astype(np.int32))
    t = layout.transpose(s)[0]
    assert np.array_equal(t.rowptr, s.rowptr) and np.array_equal(t.col, s.col)
    return s


def has_neighbour_in(g, mask):
    """[n] bool: the row stores an edge to a vertex of `mask`."""
    rows = np.repeat(np.arange(g.n_rows), np.diff(g.rowptr.astype(np.int64)))
    return np.bincount(rows[mask[g.col]], minlength=g.n_rows) > 0


PLAN = (1024, 512)           # the default hub-row plan of these graphs (threshold, chunk)
_GRAPHS = {}


def graph(name) -> layout.HostGraph:
    """"cora": symmetrised cora_like (2 708 rows, short rows); "hub": symmetrised hub_sym_graph
    without self loops (8 205 rows > 4 096, isolated empty rows, 4 hub rows of 1 128-1 800 edges);
    "long": symmetrised long_rows_graph with self loops (3 000 rows, 6 hub rows of 1 207-1 753
    edges).  Storing every edge once shortens the source graphs' longest rows."""
    if not _GRAPHS:
        _GRAPHS["cora"] = symmetrise(G.cora_like())
        _GRAPHS["hub"] = symmetrise(HG.hub_sym_graph(), loops=False)
        _GRAPHS["long"] = symmetrise(G.long_rows_graph())
        for k, g in _GRAPHS.items():
            deg = np.diff(g.rowptr.astype(np.int64))
            assert layout.split_threshold(g.n_rows, g.nnz) == PLAN[0] or k == "cora", k
            if k == "cora":
                assert deg.max() <= PLAN[0]
            else:                # hub rows under the default plan, several chunks each
                assert (deg > PLAN[0]).sum() >= 4 and 3 * PLAN[1] < deg.max() < 3000, (k, deg.max())
        h = np.diff(_GRAPHS["hub"].rowptr)
        assert _GRAPHS["hub"].n_rows > 4096 and (h == 0).sum() >= 100
    return _GRAPHS[name]


# (graph, heads, F, aR recomputed, logits past 30)
CASES = (
    ("cora", 1, 47, False, False), ("cora", 1, 47, True, True), ("cora", 3, 24, False, True),
    ("cora", 8, 256, True, False),
    ("hub", 8, 256, False, True), ("hub", 8, 256, True, False), ("hub", 1, 47, False, False),
    ("hub", 3, 24, True, True),
    ("long", 8, 64, False, False), ("long", 1, 47, True, True),
)


def case_id(c):
    return f"{c[0]}-h{c[1]}-F{c[2]}-{'rc' if c[3] else 'aR'}-{'big' if c[4] else 'plain'}"


def inputs(g, heads, F, rc, big, seed=9):
    """aL, aR [n, H], X, dY [n, F] in [-1, 1], wR [F], bR [H].  big: logits past 30, where the
    REF softmax's clamp would matter -- given aR: aL, aR in [-18, 18]; recomputed aR: wR scaled
    so that <X, wR> spreads over about +-20 and aL in [-18, 18]."""
    rng = np.random.default_rng(seed + 100 * heads + F)
    i = SimpleNamespace(heads=heads, F=F, rc=rc, big=big)
    s = 18.0 if big else 1.0
    i.aL, i.aR = E._u(rng, -s, s, g.n_rows, heads), E._u(rng, -s, s, g.n_rows, heads)
    i.X, i.dY = E._u(rng, -1, 1, g.n_rows, F), E._u(rng, -1, 1, g.n_rows, F)
    w = (40.0 if big else 0.25) / np.sqrt(F // heads)
    i.wR, i.bR = E._u(rng, -w, w, F), E._u(rng, -0.1, 0.1, heads)
    return i


def source_logits(X, wR, bR, heads):
    """float64 <X[:, head], wR[head]> + bR and its mass, [n, H]."""
    n, F = X.shape
    D = F // heads
    t = (X.astype(np.float64) * wR.astype(np.float64)[None, :]).reshape(n, heads, D)
    return t.sum(2) + bR.astype(np.float64)[None, :], np.abs(t).sum(2) + np.abs(bR.astype(np.float64))[None, :]


def _head_dot(A, B, Bm, heads):
    """<A, B>_h and sum |A| Bm per head, [n, H]."""
    n, F = A.shape
    D = F // heads
    a = A.astype(np.float64).reshape(n, heads, D)
    return (a * B.reshape(n, heads, D)).sum(2), (np.abs(a) * Bm.reshape(n, heads, D)).sum(2)


def exact_layer(g, aL, aR, X, dY, heads, slope=SLOPE):
    """The float64 layer on the symmetric graph g from fp32 inputs (aR the source logits the
    kernels used).  Namespace of Y, Ym [n, F], sma, lse [n, H], dX [n, F], daL, daR [n, H], each
    with X_mass; plus alpha, m [nnz, H] (edge (r, c) in row r's order) and dX_on_A, the REF
    backward's sum_c alpha_rc dY[c]."""
    R = E.Rows(g)
    H = heads
    z, m = E.logits(R, aL, aR, H, slope)
    mx = R.max(z)
    mx0 = np.where(np.isfinite(mx), mx, 0.0)
    p = np.exp(z - mx0[R.row])
    S = R.sum(p)
    with np.errstate(divide="ignore"):
        lse = np.where(S > 0, mx0 + np.log(np.where(S > 0, S, 1.0)), 0.0)
        alpha = p / np.where(S > 0, S, 1.0)[R.row]
    o = SimpleNamespace(R=R, alpha=alpha, m=m)
    o.Y, o.Y_mass = E._aggregate(R, alpha, X, H)
    o.Ym, o.Ym_mass = E._aggregate(R, m * alpha, X, H)
    o.sma = R.sum(m * alpha)
    o.sma_mass = o.sma
    o.lse, o.lse_mass = lse, np.where(S > 0, np.abs(mx0) + np.abs(np.log(np.where(S > 0, S, 1.0))) + 1.0, 0.0)
    gg, gm = _head_dot(dY, o.Y, o.Y_mass, H)
    s1, s1m = _head_dot(dY, o.Ym, o.Ym_mass, H)
    o.daL, o.daL_mass = s1 - gg * o.sma, s1m + gm * o.sma
    # row c's stored edge to r stands for the in-edge (r, c): alpha_rc from r's side
    zt, mt = E.logits(R, aR, aL, H, slope)                   # fl32(aR[c] + aL[r]) at row c's edge to r
    w = np.exp(zt - lse[R.col])
    o.dX, o.dX_mass = E._aggregate(R, w, dY, H)
    dXm, dXm_mass = E._aggregate(R, mt * w, dY, H)
    sg, sgm = R.sum(mt * w * gg[R.col]), R.sum(mt * w * gm[R.col])
    d2, d2m = _head_dot(X, dXm, dXm_mass, H)
    o.daR, o.daR_mass = d2 - sg, d2m + sgm
    o.dX_on_A, _ = E._aggregate(R, alpha, dY, H)
    return o


def check(tag, got, ref, g, c=None, chunk=PLAN[1]):
    """Every quantity of `got` (a dict) against the float64 layer `ref`; returns {quantity: worst
    err / mass}.  c: the constants (default C)."""
    c = C if c is None else c
    out = {}
    for k, v in got.items():
        out[k] = E.assert_bounded(f"{tag} {k}", v, getattr(ref, k), getattr(ref, k + "_mass"), c[k], g=ref.R, per="row",
                                  chunk=chunk, record=False)
    return out
