"""The exact GAT pair over gathered tables on the host (gala_cpu_gat_fwd_stats_exact_ex_f32,
gala_cpu_gat_bwd_exact_pre_ex_f32, gala_cpu_gat_bwd_exact_gather_ex_f32, the twins of the HIP
calls): bit-identity with the square pair across row partitions, the float64 layer, the square
pair unchanged from the commit before these calls, and the argument checks of both libraries."""
from __future__ import annotations

import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import _gat_exact_rect as R
import _gat_exact_ref as X
from _hub_graphs import PlannedCsr
from gala import _abi, backend
from gala import dist as gdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ("cora", "hub", "long")
_SQUARE = {}
# the golden files' case per graph: (heads, F, aR recomputed, logits past 30)
GOLDEN = {"cora": (1, 47, True, False), "hub": (3, 24, False, True), "long": (8, 256, True, False)}


def _inputs(name, shape):
    H, F, rc, big = shape
    return X.inputs(X.graph(name), H, F, rc, big)


def _square(name, shape):
    """The square pair's outputs, computed once per (graph, shape) and left unchanged."""
    key = (name, shape)
    if key not in _SQUARE:
        out = R.square_layer(backend.CpuBackend(), name, _inputs(name, shape))
        for v in out.values():
            v.setflags(write=False)
        _SQUARE[key] = out
    return _SQUARE[key]


def test_abi_has_the_table_calls():
    for lib in (_abi.lib(), _abi.cpu_lib()):
        pre = "gala_cpu_" if lib is _abi.cpu_lib() else "gala_"
        for fn in ("gat_fwd_stats_exact_ex_f32", "gat_bwd_exact_pre_ex_f32", "gat_bwd_exact_gather_ex_f32"):
            assert hasattr(lib, pre + fn), pre + fn
    assert _abi.lib().gala_abi_version() == 6


@pytest.mark.parametrize("name", GRAPHS)
def test_partitions_have_the_cases(name):
    R.check_partitions(name)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("part", range(4), ids=R.IDS)
@pytest.mark.parametrize("name", GRAPHS)
def test_partitions_are_bit_identical_to_the_square_pair(name, part, shape):
    """Every output of every rank equals the square pair's rows bit for bit, hub rows included
    (the ranks run the whole graph's plan), with aR given and recomputed."""
    world, bounds = R.partitions(name)[part]
    got, parts = R.rect_layer(backend.CpuBackend(), name, bounds, _inputs(name, shape))
    want = _square(name, shape)
    assert len(parts) == world
    for k in R.NAMES:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, name, R.IDS[part])


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("name", GRAPHS)
def test_world3_against_float64(name, shape):
    """The three-rank results within the c * mass bounds of the float64 layer (C unchanged)."""
    g = X.graph(name)
    i = _inputs(name, shape)
    got, _ = R.rect_layer(backend.CpuBackend(), name, R.partitions(name)[2][1], i)
    ref = X.exact_layer(g, i.aL, got["aR"], i.X, i.dY, i.heads)
    worst = X.check(f"rect {name} {R.shape_id(shape)}", {k: got[k] for k in X.QUANTITIES}, ref, g)
    print(name, R.shape_id(shape), worst)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("name", GRAPHS)
def test_square_pair_is_pre_plus_gather(name, shape):
    """The old entry points give the bits of the forward, the pre-pass and the gather at self_col NULL."""
    got = R.square_split(backend.CpuBackend(), name, _inputs(name, shape))
    want = _square(name, shape)
    for k in R.NAMES:
        assert np.array_equal(got[k], want[k]), (k, name)


@pytest.mark.parametrize("name", GRAPHS)
def test_square_pair_unchanged_from_the_parent(name):
    """tests/golden/gat_exact/gat_exact_square_<graph>.npz holds the square host twins' outputs of commit
    42af8ce (before the table calls), one case per graph: the sha256 of every whole output and a
    copy of its hub rows and every 32nd row.  Written on that commit by

        python tools/gat_exact_golden.py

    which calls only the square entry points; today's square pair gives the same bits."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "gat_exact", f"gat_exact_square_{name}.npz"))
    shape = GOLDEN[name]
    assert X.case_id((name,) + shape) == str(z["case"])
    got = _square(name, shape)
    rows = z["rows"]
    hub = np.flatnonzero(np.diff(X.graph(name).rowptr) > X.PLAN[0])
    assert np.isin(hub, rows).all() and rows.size > 80
    for k in R.NAMES:
        assert np.array_equal(got[k][rows], z[k]), (k, name)
        assert hashlib.sha256(np.ascontiguousarray(got[k]).tobytes()).hexdigest() == str(z[k + "_sha256"]), (k, name)


def _table_args(name="hub", H=2, F=8, bounds=(0, 2001, 6204, 8205), rank=1):
    g = X.graph(name)
    p = gdist.partition_graph(g, rank, len(bounds) - 1, bounds=np.asarray(bounds, np.int64), halo_mode="p2p")
    rng = np.random.default_rng(3)
    f = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    a = dict(p=p, H=H, F=F, aL=f(p.n, H), As=f(p.n_cols, H), Xs=f(p.n_cols, F), dY=f(p.n, F), dYs=f(p.n_cols, F),
             Y=f(p.n, F), Ym=f(p.n, F), lse=f(p.n, H), sma=f(p.n, H), sc=np.arange(p.lo, p.lo + p.n, dtype=np.int32),
             side=np.zeros(p.n_cols * H * 4 + 4, np.float32), dX=np.full((p.n, F), 7.0, np.float32),
             daL=np.full((p.n, H), 7.0, np.float32), daR=np.full((p.n, H), 7.0, np.float32))
    return a


def _P(a):
    return None if a is None else a.ctypes.data


def _calls(lib, pre, csr, a, side=None, sc="own"):
    """(forward, pre-pass, gather) statuses of one library on host arrays."""
    H, F = a["H"], a["F"]
    sc = _P(a["sc"]) if sc == "own" else sc
    side = _P(a["side"]) if side is None else side
    fwd = getattr(lib, pre + "gat_fwd_stats_exact_ex_f32")(
        csr, _P(a["aL"]), _P(a["As"]), None, None, _P(a["Xs"]), F, F, H, X.SLOPE, _P(a["Y"]), F, _P(a["lse"]),
        _P(a["Ym"]), F, _P(a["sma"]), sc, None, None)
    pre_ = getattr(lib, pre + "gat_bwd_exact_pre_ex_f32")(
        csr, _P(a["aL"]), _P(a["dY"]), F, F, H, _P(a["lse"]), _P(a["Y"]), F, _P(a["Ym"]), F, _P(a["sma"]), sc, side,
        _P(a["daL"]), None)
    gat = getattr(lib, pre + "gat_bwd_exact_gather_ex_f32")(
        csr, _P(a["As"]), _P(a["Xs"]), F, _P(a["dYs"]), F, F, H, X.SLOPE, side, sc, _P(a["dX"]), F, _P(a["daR"]), None)
    return fwd, pre_, gat


def test_argument_checks():
    """GALA_ERR_INVALID_ARG before anything runs or is launched, from both libraries: more rows
    than columns, self_col NULL on a pattern that is not square, a side table off 16 bytes; from
    the HIP library also a plan with hub rows and no workspace (the forward and the gather; the
    pre-pass is row-local and reads no plan)."""
    a = _table_args()
    p = a["p"]
    assert p.n_cols > p.n > 0 and p.lo > 0
    bad = _abi.GALA_ERR_INVALID_ARG
    tall = PlannedCsr(p.graph, 1 << 20, 512)
    tall.c.n_cols = p.n - 1                      # n_rows > n_cols
    rect = PlannedCsr(p.graph, 1 << 20, 512)     # no hub rows under this threshold
    hubs = PlannedCsr(p.graph, *X.PLAN)          # hub rows, host index arrays, no workspace
    assert hubs.n_rows_split > 0 and rect.n_rows_split == 0
    for lib, pre in ((_abi.cpu_lib(), "gala_cpu_"), (_abi.lib(), "gala_")):
        assert _calls(lib, pre, tall.ref, a) == (bad, bad, bad)
        assert _calls(lib, pre, rect.ref, a, sc=None) == (bad, bad, bad)
        _, s1, s2 = _calls(lib, pre, rect.ref, a, side=_P(a["side"]) + 4)
        assert (s1, s2) == (bad, bad)
    fwd, _, gat = _calls(_abi.lib(), "gala_", hubs.ref, a)
    assert (fwd, gat) == (bad, bad)
    assert np.all(a["dX"] == 7.0) and np.all(a["daR"] == 7.0) and np.all(a["daL"] == 7.0)
    assert _calls(_abi.cpu_lib(), "gala_cpu_", rect.ref, a) == (0, 0, 0)      # the same arguments are fine
    assert not np.any(a["dX"] == 7.0)
    # the layer refuses a graph that is not symmetric, whatever the partition
    with pytest.raises(ValueError):
        gdist.HaloGatExact(p, 8, 2, backend.CpuBackend(), None, symmetric=False)
    layer = gdist.HaloGatExact(gdist.partition_graph(X.graph("cora"), 0, 1), 8, 2, backend.CpuBackend(), None,
                               symmetric=True)
    assert layer.halo_bytes() == 0
