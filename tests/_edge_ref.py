"""TEST INFRASTRUCTURE: float64 reference of the edge family (row sum K7, SDDMM dot K9, edge
softmax forward / backward, the fused GAT forward / backward and its factored, recomputed and
statistics variants), with the mass of every element, and the one checker that bounds a
kernel's result per element against them.

Plain numpy (np.add.reduceat over rows); nothing here calls oracle/ or gala/.  Every function
returns (value, mass): mass is the float64 sum of the absolute values of every term that
enters the element.  An fp32 evaluation of the element, in whichever order, errs in
proportion to that sum, so the check is

    |got - ref| <= c * mass + floor            (assert_bounded, on every element)

with one constant c per quantity.  An absolute 1e-4 says nothing on a long row, where alpha,
d alpha, dz and the softmax backward's output are ~ 1 / degree; c * mass scales with the row.

Graphs are anything with n_rows, n_cols, rowptr, col, n_seg (layout.HostGraph, orc.Graph):
CSR, or column-tiled with n_seg rowptr blocks whose edges are stored segment after segment.
Edge arrays are [nnz, heads] (flat or not), features [rows, heads * D].

The constants C
---------------
c is measured, not derived (the exp, the divisions and a sum in an order the GPU chooses all
contribute).  The yardstick is the oracle's sequential fp32 chain (oracle/gala_oracle.c, the
restatement of the reference kernels), never the HIP kernels: the worst |oracle - float64| /
mass per quantity over every case of tests/test_edge_bounds_cpu.py::test_oracle_and_cpu_twins
(long_rows_graph() untiled and tiled, with_empty_rows(); heads 1, 3, 8 and F = 47; REF and
FIXED; plain and spotlight inputs), times 8 (three bits: the kernels regroup the same rounded
terms), rounded up to one significant digit.  Measured on the CPU
(profiles/edge_bounds_cpu.jsonl):

    quantity                                           worst oracle err / mass      c
    alpha, p, q   (softmax, GAT, the layer's q)
        plain inputs                                   2.09e-6                      2e-5
        spotlight inputs                               1.60e-5                      2e-4
    Y, Ym, sma, dX  (orc.gat_fwd, the layer's Y, dX)   2.59e-6                      3e-5
    ds, dz  (softmax backward, GAT dz)                 1.17e-6                      1e-5
    d_aL  (orc.gat_bwd, the layer's d_aL)              1.28e-7                      2e-6
    SDDMM dot                                          2.54e-7                      3e-6
    row sum                                            1.88e-6                      2e-5

"The layer" is orc.GatRefLayer, the pass-by-pass REF layer that forms alpha itself: it is the
yardstick of the kernels that recompute alpha (gat_bwd_stats, gat_bwd_fused), so their dX and
d_aL are measured with alpha's error in them; orc.gat_bwd is handed the float64 alpha rounded
to fp32, as the alpha-reading kernels are.
alpha has two constants because the oracle's error has two regimes.  The lifted edges of a
spotlit row share one logit (aL[r] + 8), and a sequential fp32 sum of hundreds of equal terms
rounds the same way at every step, a bias where different terms give a random walk: 1.60e-5
with the 16-edge-chunk spotlight set (hundreds of lifted edges per long row), 2.9e-6 with the
512-edge one, 2.09e-6 on the plain inputs.  One constant for both would leave the plain
inputs, where a missing edge is light, ten times looser than their own yardstick gives;
c_alpha(spot) picks the constant of the input set.
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import numpy as np

REF, FIXED = 0, 1                            # GALA_SOFTMAX_REF / GALA_SOFTMAX_FIXED
EPS = float(np.float32(1e-12))               # K7's per-segment epsilon, as the kernels hold it
CLAMP = float(np.float32(1e12))              # the REF softmax's exp clamp

def c_from(worst: float) -> float:
    """8 x worst, rounded up to one significant digit."""
    x = 8.0 * worst
    e = int(np.floor(np.log10(x)))
    return float(f"{int(np.ceil(x / 10.0 ** e - 1e-9))}e{e}")


# worst |oracle - float64| / mass over test_oracle_and_cpu_twins (the table above), and c
MEASURED = {"alpha": 2.09e-6, "alpha_spot": 1.60e-5, "Y": 2.59e-6, "ds": 1.17e-6, "daL": 1.28e-7, "sddmm": 2.54e-7, "row_sum": 1.88e-6}
C = {k: c_from(v) for k, v in MEASURED.items()}


def c_alpha(spot) -> float:
    """alpha's constant for an input set: spot is the spotlight chunk size, or None / 0 (plain)."""
    return C["alpha_spot"] if spot else C["alpha"]


class Rows:
    """Row of every stored edge of a CSR / column-tiled graph, and sums over rows."""

    def __init__(self, g):
        n, S = int(g.n_rows), int(g.n_seg)
        rp = np.asarray(g.rowptr).reshape(S, n + 1).astype(np.int64)
        assert (rp[:, 0] == 0).all()
        self.n, self.n_seg, self.nnz = n, S, int(np.asarray(g.col).shape[0])
        self.col = np.asarray(g.col).astype(np.int64)
        self.row = np.concatenate([np.repeat(np.arange(n), np.diff(rp[s])) for s in range(S)])
        assert self.row.shape[0] == self.nnz
        self.deg = np.bincount(self.row, minlength=n)
        self.order = np.argsort(self.row, kind="stable")          # identity when n_seg == 1
        self.start = np.concatenate([[0], np.cumsum(self.deg)])[:-1]
        self.nonempty = np.flatnonzero(self.deg)
        # position of every edge within its row (segment 0's edges first, as the kernels walk)
        self.pos = np.empty(self.nnz, np.int64)
        self.pos[self.order] = np.arange(self.nnz) - np.repeat(self.start, self.deg)

    def _reduce(self, ufunc, x, fill):
        out = np.full((self.n,) + x.shape[1:], fill, np.float64)
        if len(self.nonempty):
            out[self.nonempty] = ufunc.reduceat(x[self.order], self.start[self.nonempty], axis=0)
        return out

    def sum(self, x):
        return self._reduce(np.add, x, 0.0)

    def max(self, x):
        return self._reduce(np.maximum, x, -np.inf)


def _rows(g):
    return g if isinstance(g, Rows) else Rows(g)


def _e(a, nnz, heads):
    return np.asarray(a).reshape(nnz, heads)


def row_sum(g, v, heads=1, eps=1e-12):
    """K7: eps (once per segment) + sum_row v; mass sum |v|.  [n * heads]."""
    R = _rows(g)
    v = _e(v, R.nnz, heads).astype(np.float64)
    e = float(np.float32(eps)) * R.n_seg
    return (e + R.sum(v)).ravel(), R.sum(np.abs(v)).ravel()


def sddmm(g, A, B, heads=1):
    """K9: <A[row, head], B[col, head]>; mass sum |a| |b|.  [nnz * heads]."""
    R = _rows(g)
    F = A.shape[1]
    D = F // heads
    val, mass = np.empty((R.nnz, heads)), np.empty((R.nnz, heads))
    for h in range(heads):
        t = A[R.row, h * D:(h + 1) * D].astype(np.float64) * B[R.col, h * D:(h + 1) * D].astype(np.float64)
        val[:, h], mass[:, h] = t.sum(1), np.abs(t).sum(1)
    return val.ravel(), mass.ravel()


def _softmax(R, z, mode):
    """(p, q, alpha) of float64 logits z [nnz, H]: REF p = min(exp z, 1e12), S = sum over
    segments of (1e-12 + sum p); FIXED the stable softmax (q = 1 / sum exp(z - max))."""
    if mode == REF:
        p = np.minimum(np.exp(z), CLAMP)
        q = 1.0 / (EPS * R.n_seg + R.sum(p))
    else:
        m = R.max(z)
        p = np.exp(z - np.where(np.isfinite(m), m, 0.0)[R.row])
        with np.errstate(divide="ignore"):
            q = 1.0 / R.sum(p)                                  # an empty row has no edge to scale
    return p, q, p * q[R.row]


def softmax_fwd(g, s, heads=1, mode=REF):
    """alpha [nnz * heads]; its mass is alpha itself (one positive term over a positive sum)."""
    R = _rows(g)
    _, _, alpha = _softmax(R, _e(s, R.nnz, heads).astype(np.float64), mode)
    return alpha.ravel(), alpha.ravel()


def _softmax_bwd(R, alpha, da, da_mass, mode):
    """ds = sd - alpha (eps n_seg + sum sd), sd = alpha da, with masses through each product
    and difference; (ds, mass)."""
    sd, sdm = alpha * da, alpha * da_mass
    c = (EPS * R.n_seg if mode == REF else 0.0) + R.sum(sd)
    return sd - alpha * c[R.row], sdm + alpha * R.sum(sdm)[R.row]


def softmax_bwd(g, alpha, dalpha, heads=1, mode=REF):
    """d logits [nnz * heads]; mass |sd| + alpha sum |sd|."""
    R = _rows(g)
    d = _e(dalpha, R.nnz, heads).astype(np.float64)
    ds, m = _softmax_bwd(R, _e(alpha, R.nnz, heads).astype(np.float64), d, np.abs(d), mode)
    return ds.ravel(), m.ravel()


def _aggregate(R, w, X, heads):
    """sum_row w[e, head] X[col_e, head's columns] and the same over |X| (w >= 0)."""
    F = X.shape[1]
    D = F // heads
    val, mass = np.empty((R.n, F)), np.empty((R.n, F))
    for h in range(heads):
        x = X[R.col, h * D:(h + 1) * D].astype(np.float64) * w[:, h:h + 1]
        val[:, h * D:(h + 1) * D], mass[:, h * D:(h + 1) * D] = R.sum(x), R.sum(np.abs(x))
    return val, mass


def logits(R, aL, aR, heads, slope):
    """The fp32 logit t = fl32(aL[r] + aR[c]) formed as the (bit-exact) SDDVV forms it, then
    widened: (LeakyReLU(t) in float64, m = the LeakyReLU factor).  With the kernel's own fp32
    logit the branch of every edge is the kernel's, and no edge needs excluding."""
    t = (np.asarray(aL, np.float32).reshape(-1, heads)[R.row] + np.asarray(aR, np.float32).reshape(-1, heads)[R.col])
    assert t.dtype == np.float32
    m = np.where(t > 0, 1.0, float(np.float32(slope)))
    return t.astype(np.float64) * m, m


def gat_fwd(g, aL, aR, X, heads=1, slope=0.2, mode=REF, stats=False):
    """The fused GAT forward.  Namespace of [nnz, H] p, alpha, m; [n, H] q; [n, F] Y, Y_mass;
    with stats also Ym, Ym_mass [n, F] and sma [n, H].  Masses of p, q, alpha and sma are the
    values themselves (positive terms)."""
    R = _rows(g)
    z, m = logits(R, aL, aR, heads, slope)
    p, q, alpha = _softmax(R, z, mode)
    out = SimpleNamespace(R=R, p=p, q=q, alpha=alpha, m=m)
    out.Y, out.Y_mass = _aggregate(R, alpha, X, heads)
    if stats:
        out.Ym, out.Ym_mass = _aggregate(R, m * alpha, X, heads)
        out.sma = R.sum(m * alpha)
    return out


def gat_bwd(g, aL, aR, X, dY, alpha, heads=1, slope=0.2, mode=REF, dX=False):
    """The GAT edge backward on one pattern from a given alpha [nnz, H] (float64, or the fp32
    array handed to the kernel): da = <dY[r], X[c]> -> softmax backward -> dt = m ds ->
    d_aL = eps n_seg (REF) + sum dt.  Namespace of dz, dz_mass [nnz, H], daL, daL_mass [n, H]
    and, with dX (REF, square pattern), dX = sum alpha dY[c] with dX_mass."""
    R = _rows(g)
    _, m = logits(R, aL, aR, heads, slope)
    alpha = _e(alpha, R.nnz, heads).astype(np.float64)
    da, dam = sddmm(R, dY, X, heads)
    ds, dsm = _softmax_bwd(R, alpha, da.reshape(R.nnz, heads), dam.reshape(R.nnz, heads), mode)
    out = SimpleNamespace(R=R, dz=m * ds, dz_mass=m * dsm)
    out.daL = (EPS * R.n_seg if mode == REF else 0.0) + R.sum(out.dz)
    out.daL_mass = R.sum(out.dz_mass)
    if dX:
        out.dX, out.dX_mass = _aggregate(R, alpha, dY, heads)
    return out


def assert_bounded(name, got, ref, mass, c, floor=1e-12, g=None, per=None, chunk=None, record=True):
    """|got - ref| <= c * mass + floor on every element; nothing is masked out, and a NaN fails
    unless ref is NaN at the same place.  g (a graph or Rows) with per = "edge" ([nnz, heads]
    arrays) or "row" ([n, heads | F]; taken from a 2-D ref's shape when not given): a failure
    names the worst element's row, degree, head / column, and for an edge its position within
    the row and (chunk: the hub-row plan's chunk size) position // chunk.  GALA_TEST_RECORD=<path> appends the case's worst
    ratios as a JSON line (record=False: not for this call).  Returns the worst |err| / mass (0 / 0 counted as 0)."""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    ref = np.asarray(ref, np.float64)
    mass = np.asarray(mass, np.float64).reshape(ref.shape)
    assert c > 0 and (mass >= 0).all(), name
    err = np.abs(got - ref)
    both_nan = np.isnan(got) & np.isnan(ref)
    err = np.where(both_nan, 0.0, np.where(np.isnan(err), np.inf, err))
    bound = np.where(both_nan, 1.0, c * mass + floor)
    over = err / bound
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(err == 0, 0.0, err / mass)
    rec = {"case": name, "worst_over_bound": float(np.max(over, initial=0.0)),
           "worst_err_over_mass": float(np.max(rel[np.isfinite(rel)], initial=0.0))}
    path = os.environ.get("GALA_TEST_RECORD")
    if path and record:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
    if not rec["worst_over_bound"] <= 1.0:
        i = int(np.argmax(over))
        where = f"flat index {i}"
        if g is not None:
            R = _rows(g)
            if per is None and ref.ndim == 2 and R.nnz != R.n:
                per = "edge" if ref.shape[0] == R.nnz else "row" if ref.shape[0] == R.n else None
            if per == "edge":
                w = ref.size // R.nnz
                e, h = i // w, i % w
                r, k = int(R.row[e]), int(R.pos[e])
                where = f"edge {e}: row {r}, degree {int(R.deg[r])}, head {h}, position {k} in its row"
                if chunk:
                    where += f", chunk {k // chunk} of {-(-int(R.deg[r]) // chunk)} ({chunk}-edge chunks)"
            elif per == "row":
                w = ref.size // R.n
                r, k = i // w, i % w
                where = f"row {r}, degree {int(R.deg[r])}, head / column {k} of {w}"
                if chunk:
                    where += f", {-(-int(R.deg[r]) // chunk)} chunks of {chunk} edges"
        raise AssertionError(f"{name}: |got - ref| = {err.flat[i]:.3e} > {c:g} * mass ({mass.flat[i]:.3e}) + {floor:g} "
                             f"= {bound.flat[i]:.3e} (x{over.flat[i]:.3g}) at {where}; got {got.flat[i]!r}, "
                             f"ref {ref.flat[i]!r}; {int((over > 1).sum())} of {over.size} elements over")
    return rec["worst_err_over_mass"]


def spotlight_edges(g, chunk, longer_than=64):
    """Edge indices at positions 0, deg - 1 and k * chunk - 1, k * chunk (every chunk boundary
    inside the row) of every row longer than `longer_than` edges, and the number of them per
    row [n]."""
    R = _rows(g)
    deg = R.deg[R.row]
    k = R.pos
    hit = (deg > longer_than) & ((k == 0) | (k == deg - 1) | (k % chunk == 0) | (k % chunk == chunk - 1))
    return np.flatnonzero(hit), np.bincount(R.row[hit], minlength=R.n)


# ---- the inputs of the bound tests (CPU and GPU files) --------------------------------------
SLOPE = 0.2
# a spotlit edge's share of its row is at least SPOT_WEIGHT / (lifted edges of the row).  Softmax:
# e^9 = 8 103 against deg * 3.34 on average from the others (2 600 edges: 8 684, one more
# "edge"); GAT: e^(aL + 8) >= e^7 = 1 097 against deg * ~2.2 (5 700: five more).
SPOT_WEIGHT = 0.4


def _u(rng, lo, hi, *shape):
    return rng.uniform(lo, hi, shape).astype(np.float32)


def edge_inputs(g, heads, F, spot=None, seed=5):
    """Inputs of every op on graph g, in the ranges the suite uses everywhere: s in [-3, 3], d,
    v_signed in [-1, 1], v_pos in [0, 1] [nnz, H]; aL, aR [n, H], X, dY [n, F] in [-1, 1]; wR [F],
    bR [H].  spot (a chunk size): the spotlight set -- the edges at positions 0, deg - 1, k spot
    - 1 and k spot of every row longer than 64 edges get s = +9 and their columns aR = +8 (so
    every edge of such a column is lifted, in whichever row) -- with .spot = (edges, number per
    row)."""
    R = Rows(g)
    rng = np.random.default_rng(seed + 100 * heads + F)
    i = SimpleNamespace(R=R, heads=heads, F=F, spot=None)
    i.s, i.d = _u(rng, -3, 3, R.nnz, heads), _u(rng, -1, 1, R.nnz, heads)
    i.v_pos, i.v_signed = _u(rng, 0, 1, R.nnz, heads), _u(rng, -1, 1, R.nnz, heads)
    i.aL, i.aR = _u(rng, -1, 1, g.n_rows, heads), _u(rng, -1, 1, g.n_cols, heads)
    i.X, i.dY = _u(rng, -1, 1, g.n_cols, F), _u(rng, -1, 1, g.n_rows, F)
    i.wR, i.bR = _u(rng, -0.25, 0.25, F), _u(rng, -0.1, 0.1, heads)
    if spot:
        e, per_row = spotlight_edges(R, spot)
        i.s[e] = 9.0
        i.aR[R.col[e]] = 8.0
        i.spot = (e, per_row)
    return i


def spot_check(i, alpha, gat):
    """On the float64 alpha: every lifted edge of a long row (softmax: the spotlit edges; GAT:
    every edge whose column is lifted) carries at least SPOT_WEIGHT / (their number in its row)
    of the row's weight, and never less than 3 x the spotlight alpha constant: one of them
    missing from, or doubled in, a denominator moves every alpha of the row by that share.
    On long_rows_graph() the smallest share is 1.6e-2 with the 512-edge-chunk set (80 c), 1.4e-3
    with the 32-edge one (7 c) and 7.6e-4 with the 16-edge one (3.8 c; aR = +8 then lifts 45 %
    of all columns, so a 2 600-edge row holds ~1 200 lifted edges); 7.6e-2, 6.1e-3 and 3.1e-3
    for the softmax, whose lift touches the spotlit edges alone.  Returns the smallest share."""
    R = i.R
    if gat:
        lit = (R.deg[R.row] > 64) & (i.aR[R.col, 0] == 8.0)
    else:
        lit = np.zeros(R.nnz, bool)
        lit[i.spot[0]] = True
    k = np.bincount(R.row[lit], minlength=R.n)
    a = alpha.reshape(R.nnz, -1)[lit]
    w = a * k[R.row[lit]][:, None]
    assert lit.sum() >= 2 * (R.deg > 64).sum() and w.min() >= SPOT_WEIGHT, w.min()
    assert a.min() >= 3 * C["alpha_spot"], a.min()
    return float(a.min())
