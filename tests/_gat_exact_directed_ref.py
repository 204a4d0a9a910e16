"""TEST INFRASTRUCTURE: float64 reference of the exact GAT layer on a DIRECTED pattern (the forward
gala_gat_fwd_stats_exact_f32 on A, the backward gala_gat_bwd_stats_exact_t_f32 whose gather pass
walks A^T), with the mass of every element, the graphs and inputs of its tests, and the constants
of its bounds.

The formulas are tests/_gat_exact_ref.py's; the backward's column sums run over the in-edges of
c taken from A's explicit edge list, {r : (r, c) in A}:

    dX[c] = sum_r alpha_rc dY[r],  dXm[c] = sum_r m alpha_rc dY[r],  sg[c] = sum_r m alpha_rc g[r],
    d_aR[c] = <dXm[c], X[c]>_h - sg[c]

tests/test_gat_exact_directed_cpu.py::test_reference_is_the_derivative checks them against
torch.autograd of the dense float64 layer on a directed graph.

Bounds: |got - ref| <= c * mass + 1e-12 on every element (_edge_ref.assert_bounded), c = 8 x the
host twins' worst |twin - float64| / mass over CASES rounded up to one digit (_edge_ref.c_from),
measured by test_gat_exact_directed_cpu.py::test_twins_against_float64
(profiles/gat_exact_directed_bounds_cpu.jsonl).  Where the directed worst is no larger than the
symmetric pair's (_gat_exact_ref.MEASURED), the symmetric constant is reused:

    quantity      worst twin err / mass      symmetric worst      c
    Y             2.65e-6                    8.22e-7              3e-5
    Ym            2.30e-6                    8.22e-7              2e-5
    sma           2.02e-6                    1.12e-6              2e-5
    lse           1.86e-7                    1.58e-7              2e-6
    dX            3.57e-6                    3.74e-6              3e-5  (reused)
    d_aL          4.35e-7                    1.42e-7              4e-6
    d_aR          3.33e-6                    2.60e-6              3e-5

The forward quantities are the unchanged forward's.  Every maximum but sma's and lse's is case
rmat-h2-F8-rc-big's: 2 heads of 4 columns, a shape the symmetric cases do not have, on the graph
with the longest rows, with a recomputed aR and logits past 30 (sma, lse: rmat-h8-F256-rc-plain).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import _edge_ref as E
import _gat_exact_ref as X
import _graphs as G
from gala import backend, layout

SLOPE = X.SLOPE
QUANTITIES = X.QUANTITIES
PLAN = X.PLAN                # (1024, 512): a hub row has at least 3 chunks
# worst |host twin - float64| / mass over CASES (test_twins_against_float64)
MEASURED = {"Y": 2.65e-6, "Ym": 2.30e-6, "sma": 2.02e-6, "lse": 1.86e-7, "dX": 3.57e-6, "daL": 4.35e-7, "daR": 3.33e-6}
C = {k: (X.C[k] if v <= X.MEASURED[k] else E.c_from(v)) for k, v in MEASURED.items()}


def edges(g):
    """(row, col) of every stored edge, int64."""
    return np.repeat(np.arange(g.n_rows, dtype=np.int64), np.diff(g.rowptr.astype(np.int64))), g.col.astype(np.int64)


def simple(n, src, dst) -> layout.HostGraph:
    """The CSR of the distinct edges (src, dst): rows sorted, columns strictly ascending."""
    key = np.unique(np.asarray(src, np.int64) * n + np.asarray(dst, np.int64))
    return layout.csr_build(n, n, (key // n).astype(np.int32), (key % n).astype(np.int32))


def in_edges(g):
    """A's edges regrouped by column, from the edge list alone (no library transpose): a CSR-like
    namespace whose row c lists, ascending, the rows r with (r, c) in A."""
    r, c = edges(g)
    o = np.lexsort((r, c))
    rp = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=g.n_rows))]).astype(np.int64)
    return SimpleNamespace(n_rows=g.n_rows, n_cols=g.n_rows, n_seg=1, rowptr=rp, col=r[o])


def directed(g, keep, seed) -> layout.HostGraph:
    """A generator's graph made directed: its distinct edges, each stored direction kept with
    probability `keep` independently (so (u, v) often stays without (v, u))."""
    r, c = edges(g)
    key = np.unique(r * g.n_rows + c)
    key = key[np.random.default_rng(seed).random(key.shape[0]) < keep]
    return simple(g.n_rows, key // g.n_rows, key % g.n_rows)


def uniform_graph(seed=3) -> layout.HostGraph:
    """300 rows, uniform and directed: rows 150..199 empty, columns 100..139 empty (vertices 150..
    199 have in-edges only, 100..139 out-edges only), vertex 299 isolated."""
    rng = np.random.default_rng(seed)
    n = 300
    src, dst = rng.integers(0, n - 1, 14000), rng.integers(0, n - 1, 14000)
    ok = ~((src >= 150) & (src < 200)) & ~((dst >= 100) & (dst < 140))
    return simple(n, src[ok], dst[ok])


def split_hub_graph(seed=5) -> layout.HostGraph:
    """3 000 rows: row 7 stores 1 500 edges (a hub of A; vertex 7 has a handful of in-edges) and
    column 11 is stored by 1 300 rows (a hub of A^T; row 11 is short); every other row 0..8."""
    rng = np.random.default_rng(seed)
    n = 3000
    deg = rng.integers(0, 9, n)
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, src.shape[0])
    others = np.setdiff1d(np.arange(n), [7, 11])
    hub_out = rng.choice(others, 1500, replace=False)
    hub_in = rng.choice(others, 1300, replace=False)
    keep = (dst != 11) & (src != 7)
    src = np.concatenate([src[keep], np.full(1500, 7), hub_in])
    dst = np.concatenate([dst[keep], hub_out, np.full(1300, 11)])
    return simple(n, src, dst)


_GRAPHS = {}


def graph(name) -> layout.HostGraph:
    """"uni": uniform_graph; "rmat": the 4 096-row R-MAT generator's graph made directed (about
    121 000 edges), vertex 0 a hub row of 3 chunks in A and in A^T under PLAN; "split":
    split_hub_graph.  None equals its transpose."""
    if not _GRAPHS:
        _GRAPHS.update(_checked_graphs())
    return _GRAPHS[name]


def _checked_graphs():
    """The three graphs, with what the tests rely on asserted from the built arrays."""
    gs = {"uni": uniform_graph(), "rmat": directed(layout.gen_graph("rmat", 4096, 120000, seed=7), 0.75, 1),
          "split": split_hub_graph()}
    thr, chunk = PLAN
    deg = {}
    for k, g in gs.items():
        t = transposed(g)
        assert not (np.array_equal(t.rowptr, g.rowptr) and np.array_equal(t.col, g.col)), k
        r, c = edges(g)
        assert np.unique(r * g.n_rows + c).shape[0] == g.nnz, k
        deg[k] = (np.diff(g.rowptr), np.diff(t.rowptr))
    out, inn = deg["uni"]
    assert (out == 0).sum() >= 50 and (inn == 0).sum() >= 40 and ((out > 0) & (inn == 0)).sum() >= 30
    assert ((out == 0) & (inn > 0)).sum() >= 40 and out.max() <= thr and inn.max() <= thr
    out, inn = deg["rmat"]
    assert out.max() > 2 * chunk and inn.max() > 2 * chunk and (out > thr).sum() >= 1 and (inn > thr).sum() >= 1
    out, inn = deg["split"]
    assert out[7] == 1500 and inn[7] <= 20 and inn[11] == 1300 and out[11] <= 20
    assert (out > thr).sum() == 1 and (inn > thr).sum() == 1
    return gs


_T = {}


def transposed(g) -> layout.HostGraph:
    """layout.transpose(g), kept per graph object."""
    if id(g) not in _T:
        _T[id(g)] = (g, layout.transpose(g)[0])
    return _T[id(g)][1]


# (graph, heads, F, aR recomputed, logits past 30): 8 x 32, 1 x 47 (the padded path) and 2 x 4
CASES = (
    ("uni", 8, 256, False, True), ("uni", 1, 47, True, False), ("uni", 2, 8, False, True),
    ("rmat", 8, 256, True, False), ("rmat", 1, 47, False, True), ("rmat", 2, 8, True, True),
    ("split", 8, 256, False, False), ("split", 1, 47, True, True), ("split", 2, 8, False, True),
)
case_id = X.case_id
inputs = X.inputs


def directed_layer(g, aL, aR, X_, dY, heads, slope=SLOPE):
    """The float64 layer on the directed graph g from fp32 inputs (aR: the source logits the
    kernels used).  Namespace of Y, Ym [n, F], sma, lse [n, H], dX [n, F], daL, daR [n, H], each
    with X_mass; alpha, m [nnz, H] in A's edge order; R (A's rows) and RT (the in-edges)."""
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
    o.Y, o.Y_mass = E._aggregate(R, alpha, X_, H)
    o.Ym, o.Ym_mass = E._aggregate(R, m * alpha, X_, H)
    o.sma = R.sum(m * alpha)
    o.sma_mass = o.sma
    o.lse, o.lse_mass = lse, np.where(S > 0, np.abs(mx0) + np.abs(np.log(np.where(S > 0, S, 1.0))) + 1.0, 0.0)
    gg, gm = X._head_dot(dY, o.Y, o.Y_mass, H)
    s1, s1m = X._head_dot(dY, o.Ym, o.Ym_mass, H)
    o.daL, o.daL_mass = s1 - gg * o.sma, s1m + gm * o.sma
    # the in-edges of c: entry (c, r) of RT stands for the edge (r, c) of A, alpha_rc from r's side
    RT = E.Rows(in_edges(g))
    o.RT = RT
    zt, mt = E.logits(RT, aR, aL, H, slope)                  # fl32(aR[c] + aL[r]) = fl32(aL[r] + aR[c])
    w = np.exp(zt - lse[RT.col])
    o.dX, o.dX_mass = E._aggregate(RT, w, dY, H)
    dXm, dXm_mass = E._aggregate(RT, mt * w, dY, H)
    sg, sgm = RT.sum(mt * w * gg[RT.col]), RT.sum(mt * w * gm[RT.col])
    d2, d2m = X._head_dot(X_, dXm, dXm_mass, H)
    o.daR, o.daR_mass = d2 - sg, d2m + sgm
    return o


FWD = ("Y", "Ym", "sma", "lse", "daL")     # indexed by A's rows; dX and daR by A^T's


def check(tag, got, ref, c=None, chunk=PLAN[1]):
    """Every quantity of `got` (a dict) against the float64 layer `ref`; returns {quantity: worst
    err / mass}.  A failure names the row of the pattern the quantity was summed over."""
    c = C if c is None else c
    out = {}
    for k, v in got.items():
        out[k] = E.assert_bounded(f"{tag} {k}", v, getattr(ref, k), getattr(ref, k + "_mass"), c[k],
                                  g=ref.R if k in FWD else ref.RT, per="row", chunk=chunk, record=False)
    return out


# ---- the host twins of a case, and the patterns that are no transpose pair ---------------------
t = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def twin_layer(be, cg, cgT, i, H):
    """The host twins' forward on cg and directed backward over cgT: ({quantity: array}, aR used)."""
    aL, Xt, dY = t(i.aL), t(i.X), t(i.dY)
    if i.rc:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(cg, aL, None, Xt, H, SLOPE, wR=t(i.wR), bR=t(i.bR))
    else:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(cg, aL, t(i.aR), Xt, H, SLOPE)
    dX, daL, daR = be.gat_bwd_stats_exact_t(cg, cgT, aL, aR, Xt, dY, lse, Y, Ym, sma, H, SLOPE)
    return dict(Y=Y.numpy(), Ym=Ym.numpy(), sma=sma.numpy(), lse=lse.numpy(), dX=dX.numpy(), daL=daL.numpy(),
                daR=daR.numpy()), aR.numpy()


_TWIN = {}


def twin_case(case):
    """The host twins' layer and the float64 layer of a case, computed once per process."""
    if case not in _TWIN:
        name, H, F, rc, big = case
        g = graph(name)
        i = inputs(g, H, F, rc, big)
        be = backend.CpuBackend()
        cg, cgT = be.graph(g), be.graph(transposed(g))
        cg.set_split_plan(*PLAN)
        cgT.set_split_plan(*PLAN)
        got, aR = twin_layer(be, cg, cgT, i, H)
        _TWIN[case] = (g, i, directed_layer(g, i.aL, aR, i.X, i.dY, H), got, aR.reshape(g.n_rows, H))
    return _TWIN[case]


def negatives(g, gT):
    """{name: (a, at)}: patterns that are no transpose pair, each one edit away from (g, gT)."""
    n = g.n_rows
    rp, col = gT.rowptr.astype(np.int32), gT.col.astype(np.int32)
    deg = np.diff(rp)
    mk = lambda rowptr, c: layout.HostGraph(n, n, np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(c, np.int32))
    out = {}
    # one edge moved to another row: row r's last edge handed to row r + 1 (columns stay ascending)
    r = next(r for r in range(n - 1) if deg[r] >= 2 and (deg[r + 1] == 0 or col[rp[r + 1]] > col[rp[r + 1] - 1]))
    rp2 = rp.copy()
    rp2[r + 1] -= 1
    out["moved"] = (g, mk(rp2, col))
    # one edge duplicated in place of another (same nnz): a row's second column := its first
    r = int(np.flatnonzero(deg >= 3)[0])
    c2 = col.copy()
    c2[rp[r] + 1] = c2[rp[r]]
    out["duplicate"] = (g, mk(rp, c2))
    # two columns of a row swapped
    c3 = col.copy()
    c3[rp[r]], c3[rp[r] + 1] = col[rp[r] + 1], col[rp[r]]
    out["swapped"] = (g, mk(rp, c3))
    # nnz differing by one: the last edge dropped
    last = int(np.flatnonzero(deg)[-1])
    rp4 = rp.copy()
    rp4[last + 1:] -= 1
    out["nnz"] = (g, mk(rp4, col[:-1]))
    # a column index out of range
    for bad in (n, 2 ** 31 - 1, -1):
        c5 = col.copy()
        c5[rp[r] + deg[r] - 1] = bad
        out[f"range{bad}"] = (g, mk(rp, c5))
    # row offsets that leave the array: followed nowhere, counted
    rp6 = rp.copy()
    rp6[n // 2] = 2 ** 30
    out["offsets"] = (g, mk(rp6, col))
    # a replaced, not moved, edge: at stays well-formed, one edge of a is missing from it
    c7 = col.copy()
    k = rp[r] + deg[r] - 1
    c7[k] = col[k] + 1 if col[k] + 1 < n and col[k] + 1 not in col[rp[r]:k] else col[k] - 1
    assert c7[k] not in col[rp[r]:rp[r + 1]] and (deg[r] < 2 or c7[k] > col[k - 1])
    out["replaced"] = (g, mk(rp, c7))
    # a itself is not a transpose of a directed pattern
    out["self"] = (g, g)
    return out


# ---- gala_csr_is_transpose_i32's grid cap, after tests/_rounds.py ---------------------------------
# k_csr_is_transpose: one item per thread per round, at most kCheckMaxBlocks = 1024 workgroups
# (csrc/csr_check.hip:23; the launch: csr_check.hip:106-107) of kBlock = 256 threads
# (csrc/gala_internal.h:17); the loop: csr_check.hip:60
CHECK_ROUND = 1024 * 256


def check_round_from_source() -> int:
    """Items per round as the launch code has them now: kCheckMaxBlocks * kBlock parsed from the
    sources, so a changed cap fails the tests' assertion instead of leaving them in one round."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "gala-gnn-acceleration-language_amd", "csrc")
    cap = re.search(r"constexpr int kCheckMaxBlocks = (\d+);", open(os.path.join(csrc, "csr_check.hip")).read())
    blk = re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(csrc, "gala_internal.h")).read())
    return int(cap.group(1)) * int(blk.group(1))


# ---- a directed dataset for the compiled programs -------------------------------------------------

def directed_npy(path, n=500, m=3000, feat=64, classes=7, seed=11):
    """A directed graph (random arcs + self loops, A^T != A) whose edges are DISTINCT -- so that
    its transpose has strictly ascending rows and gala_csr_is_transpose_i32 says yes -- with
    features, labels and masks in the reference's npy format (as test_dsl_cpu_run._directed_npy,
    which keeps duplicates).  Returns the number of edges."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, n, m), np.arange(n)]).astype(np.int64)
    dst = np.concatenate([(src[:m] + rng.integers(1, 50, m)) % n, np.arange(n)]).astype(np.int64)
    key = np.unique(src * n + dst)
    path.mkdir()
    np.save(path / "Adj_src.npy", np.concatenate([[n, n], key // n]).astype(np.uint32))
    np.save(path / "Adj_dst.npy", (key % n).astype(np.uint32))
    np.save(path / "Feat.npy", rng.uniform(-1, 1, (n, feat)).astype(np.float32))
    np.save(path / "Lab.npy", rng.integers(0, classes, (n, 1)).astype(np.int64))
    train = rng.random(n) < 0.4
    np.save(path / "TnMsk.npy", train.astype(np.int32).reshape(-1, 1))
    np.save(path / "VlMsk.npy", np.zeros((n, 1), np.int32))
    np.save(path / "TsMsk.npy", (~train).astype(np.int32).reshape(-1, 1))
    return int(key.shape[0])


def run_directed_fixed(tmp_path, switch, *extra):
    """tests/dsl/gat_directed_fixed.txt's program for one epoch on directed_npy's graph with
    GALA_GAT_EXACT_DIRECTED set to `switch` ("1", "0" or None: unset); its dump."""
    import os
    import subprocess
    import _ir_ref as ref
    from _dsl_check import PKG
    exe = os.path.join(PKG, "progs", "gat_directed_fixed", "gala_prog")
    assert os.path.exists(exe), "run tools/build_dsl_progs.py (build()) first"
    data = tmp_path / "Data"
    if not data.exists():
        directed_npy(data)
    env = {k: v for k, v in os.environ.items() if k != "GALA_GAT_EXACT_DIRECTED"}
    if switch is not None:
        env["GALA_GAT_EXACT_DIRECTED"] = switch
    dump = tmp_path / f"switch_{switch}.dump"
    r = subprocess.run([exe, "--data", str(data), "--seed", "3", "--iters", "1", "--dump", str(dump), *extra],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return ref.read_dump(str(dump))


def check_directed_fixed_program(tmp_path, *extra):
    """The program with the switch on meets the float64 executor of its IR (prediction, loss,
    every weight gradient), on a graph the transpose test accepts; and it took the directed pair:
    the attention Linears of the SECOND layer (efc2, efc3: their gradients depend on no other
    layer's backward, so that layer did switch) and of the first (efc0, efc1: these also see the
    second layer's dX, so their other bits alone do not single out the first layer -- its
    gradients are held to the float64 executor like the rest) get other bits than with the
    switch off or unset, which are the alpha-storing path's and equal each other."""
    from _dsl_check import check_against_ir
    on = run_directed_fixed(tmp_path, "1", *extra)
    off, unset = run_directed_fixed(tmp_path, "0", *extra), run_directed_fixed(tmp_path, None, *extra)
    rp, col = on["rowptr"], on["col"]
    n = len(rp) - 1
    key = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * n + col
    assert np.unique(key).shape[0] == key.shape[0] and not np.array_equal(np.diff(rp), np.bincount(col, minlength=n))
    check_against_ir("gat_directed_fixed", on)
    check_against_ir("gat_directed_fixed", off)
    grads = [k for k in on if k.startswith("grad:")]
    assert all(np.array_equal(off[k], unset[k]) for k in grads)
    for k in ("grad:efc0.weight", "grad:efc1.weight", "grad:efc2.weight", "grad:efc3.weight"):
        assert not np.array_equal(on[k], off[k]), k
    return on, off
