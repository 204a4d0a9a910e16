"""TEST INFRASTRUCTURE: the exact GAT pair over a row partition, run as one process.

The ranks of gala.dist.partition_graph (p2p tables [lower halo | own rows | higher halo]) run one
after another on the table entry points (gala_gat_fwd_stats_exact_ex_f32, gala_gat_bwd_exact_pre_ex_f32,
gala_gat_bwd_exact_gather_ex_f32 or their host twins, through a gala.backend), the dY rows and the
side lines of the halo rows copied between the ranks' tables by hand -- what gala.dist.HaloGatExact
does over a communicator.  Shared by tests/test_gat_exact_rect_cpu.py, tests/test_dist_halo_gat_exact_cpu.py
and tests/test_gpu_gat_exact_rect.py; graphs, inputs and bounds are those of tests/_gat_exact_ref.py.
"""
from __future__ import annotations

import numpy as np
import torch

import _gat_exact_ref as X
from _gat_rect import PARTITION_IDS, PARTITIONS, halo_lists, make_parts

NAMES = ("Y", "lse", "Ym", "sma", "aR", "dX", "daL", "daR")
# (heads, F, aR recomputed, logits past 30)
SHAPES = ((8, 256, True, False), (1, 47, False, True), (3, 24, True, True), (3, 24, False, False))

# "hub" has the 8 205 rows of _gat_rect.PARTITIONS; the analogous cuts of "cora" (2 708 rows) and
# "long" (3 000 rows): uneven halves with odd row counts, a middle rank with halo rows on both
# sides, a middle rank that owns no row
_PARTS = {
    "hub": PARTITIONS,
    "cora": ((1, (0, 2708)), (2, (0, 1355, 2708)), (3, (0, 701, 2004, 2708)), (3, (0, 1349, 1349, 2708))),
    "long": ((1, (0, 3000)), (2, (0, 1501, 3000)), (3, (0, 667, 2102, 3000)), (3, (0, 1499, 1499, 3000))),
}
IDS = PARTITION_IDS


def partitions(name):
    return _PARTS[name]


def plan_of(name):
    """The hub graphs run under the default plan of tests/_gat_exact_ref.py; "cora" has no hub row."""
    return None if name == "cora" else X.PLAN


def shape_id(s):
    return f"h{s[0]}-F{s[1]}-{'rc' if s[2] else 'aR'}-{'big' if s[3] else 'plain'}"


def check_partitions(name):
    """What the partition tests rely on, from the partitions' own arrays: a rank with lo > 0 and
    halo rows above its own block too, a rank whose row count is no multiple of 8, a rank without
    rows, and on the hub graphs a hub row (longer than the plan's threshold) that reads a column
    outside its rank's own block."""
    g = X.graph(name)
    both = odd = empty = far_hub = False
    for world, bounds in partitions(name):
        parts = make_parts(g, bounds)
        assert len(parts) == world and sum(p.n for p in parts) == g.n_rows
        for p in parts:
            assert p.own_offset() == p.lo and p.graph.n_rows == p.n and p.graph.n_cols == p.n_cols >= p.n
            both |= p.lo > 0 and p.lo + p.n < p.n_cols
            odd |= p.n % 8 != 0
            empty |= p.n == 0
            if plan_of(name) and world > 1 and p.n:
                assert p.split_threshold == X.PLAN[0]
                rp = p.graph.rowptr.astype(np.int64)
                for r in np.flatnonzero(np.diff(rp) > X.PLAN[0]):
                    c = p.graph.col[rp[r]:rp[r + 1]]
                    far_hub |= bool(((c < p.lo) | (c >= p.lo + p.n)).any())
    assert both and odd and empty
    assert far_hub or plan_of(name) is None


def _t(be, a):
    if a.size == 0:      # numpy gives an empty slice zero strides; the calls take ld >= F
        return torch.empty(a.shape, dtype=torch.from_numpy(a[:0].copy()).dtype, device=be.device)
    return torch.from_numpy(np.ascontiguousarray(a)).to(be.device)


def _graph(be, hg, plan):
    if be.name == "cpu":
        cg = be.graph(hg)
        if plan:
            cg.set_split_plan(*plan)
        return cg
    return be.graph(hg, split=plan[0] if plan else False)


def _np(d, n):
    return {k: v.detach().cpu().numpy().reshape(n, -1) for k, v in d.items()}


def square_layer(be, name, i):
    """The square pair (gala_gat_{fwd,bwd}_stats_exact_f32) on the whole graph: {NAMES: [n, -1]}."""
    g = X.graph(name)
    G = _graph(be, g, plan_of(name))
    H = i.heads
    aL, Xt, dY = _t(be, i.aL), _t(be, i.X), _t(be, i.dY)
    if i.rc:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(G, aL, None, Xt, H, X.SLOPE, wR=_t(be, i.wR), bR=_t(be, i.bR))
    else:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(G, aL, _t(be, i.aR), Xt, H, X.SLOPE)
    dX, daL, daR = be.gat_bwd_stats_exact(G, aL, aR, Xt, dY, lse, Y, Ym, sma, H, X.SLOPE, symmetric=True)
    return _np(dict(Y=Y, lse=lse, Ym=Ym, sma=sma, aR=aR, dX=dX, daL=daL, daR=daR), g.n_rows)


def square_split(be, name, i):
    """The table calls at self_col None on the whole (square) graph: forward, pre-pass, gather."""
    g = X.graph(name)
    G = _graph(be, g, plan_of(name))
    H, n = i.heads, g.n_rows
    aL, Xt, dY = _t(be, i.aL), _t(be, i.X), _t(be, i.dY)
    if i.rc:
        aR = torch.empty((n, H), device=be.device)
        Y, lse, Ym, sma = be.gat_stats_exact_table(G, aL, None, Xt, H, X.SLOPE, None, aR, wR=_t(be, i.wR),
                                                   bR=_t(be, i.bR))
    else:
        aR = _t(be, i.aR)
        Y, lse, Ym, sma = be.gat_stats_exact_table(G, aL, aR, Xt, H, X.SLOPE, None, None)
    side = torch.empty((n, 4 * H), device=be.device)
    daL = be.gat_bwd_exact_pre_table(G, aL, dY, lse, Y, Ym, sma, H, None, side)
    dX, daR = be.gat_bwd_exact_gather_table(G, aR, Xt, dY, side, H, X.SLOPE, None)
    return _np(dict(Y=Y, lse=lse, Ym=Ym, sma=sma, aR=aR, dX=dX, daL=daL, daR=daR), n)


def rect_layer(be, name, bounds, i, plan="default"):
    """The table calls over the partition `bounds` of graph `name`, rank after rank: every rank's
    forward over its gathered X (and aR) table, its pre-pass, the halo rows' dY and side lines
    copied from their owners' tables, the gather pass.  Returns the concatenated {NAMES: [n, -1]}
    and the partitions."""
    g = X.graph(name)
    plan = plan_of(name) if plan == "default" else plan
    parts = make_parts(g, bounds)
    H, F = i.heads, i.F
    nan = float("nan")
    ranks = []
    for p in parts:
        gl = p.xs_to_global()
        own = slice(p.r0, p.r0 + p.n)
        r = dict(p=p, G=_graph(be, p.graph, plan), sc=_t(be, np.arange(p.lo, p.lo + p.n, dtype=np.int32)),
                 aL=_t(be, i.aL[own]), Xs=_t(be, i.X[gl]), dY=_t(be, i.dY[own]))
        if i.rc:
            r["As"] = torch.full((p.n_cols, H), nan, device=be.device)
            out = be.gat_stats_exact_table(r["G"], r["aL"], None, r["Xs"], H, X.SLOPE, r["sc"], r["As"],
                                           wR=_t(be, i.wR), bR=_t(be, i.bR))
        else:
            r["As"] = _t(be, i.aR[gl])
            out = be.gat_stats_exact_table(r["G"], r["aL"], r["As"], r["Xs"], H, X.SLOPE, r["sc"], None)
        r["Y"], r["lse"], r["Ym"], r["sma"] = out
        # the pre-pass: the own rows' side lines into the table's own block; halo lines missing (NaN)
        r["Ss"] = torch.full((p.n_cols, 4 * H), nan, device=be.device)
        r["dYs"] = torch.full((p.n_cols, F), nan, device=be.device)
        r["dYs"][p.lo:p.lo + p.n] = r["dY"]
        r["daL"] = be.gat_bwd_exact_pre_table(r["G"], r["aL"], r["dY"], r["lse"], r["Y"], r["Ym"], r["sma"], H,
                                              r["sc"], r["Ss"])
        ranks.append(r)
    for dst, src, drows, srows in halo_lists(parts):
        d, s = torch.from_numpy(drows.astype(np.int64)).to(be.device), torch.from_numpy(srows.astype(np.int64)).to(be.device)
        for k in ("Ss", "dYs"):
            ranks[dst][k][d] = ranks[src][k][s]
    for r in ranks:
        p = r["p"]
        assert not bool(torch.isnan(r["Ss"]).any()) and not bool(torch.isnan(r["dYs"]).any())
        r["dX"], r["daR"] = be.gat_bwd_exact_gather_table(r["G"], r["As"], r["Xs"], r["dYs"], r["Ss"], H, X.SLOPE,
                                                          r["sc"])
        r["aR"] = r["As"][p.lo:p.lo + p.n]
    width = dict(Y=F, Ym=F, dX=F)
    cat = {k: np.concatenate([r[k].detach().cpu().numpy().reshape(r["p"].n, width.get(k, H)) for r in ranks])
           for k in NAMES}
    return cat, parts
