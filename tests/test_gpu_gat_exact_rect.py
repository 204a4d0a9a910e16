"""The exact GAT pair over gathered tables on the GPU (gala_gat_fwd_stats_exact_ex_f32,
gala_gat_bwd_exact_pre_ex_f32, gala_gat_bwd_exact_gather_ex_f32) through the one-process helper of
tests/_gat_exact_rect.py: every partition bit for bit against the square GPU pair, and against the
float64 layer at the bounds of tests/_gat_exact_ref.py.

Shapes: "hub" (8 205 rows, hub rows of 1 128-1 800 edges: several 512-edge chunks each, read
across ranks) under the four partitions of tests/_gat_rect.py, and "cora" (2 708 rows) under its
own -- the smallest fixtures that reach hub chunks whose columns sit on other ranks, an own block
that starts past table row 0, row counts that are no multiple of the row group, and an empty launch."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import _gat_exact_rect as R
import _gat_exact_ref as X
from gala import backend

pytestmark = pytest.mark.gpu
SHAPES = ((8, 256, True, False), (1, 47, False, True), (3, 24, True, True))
_SQUARE = {}


def _inputs(name, shape):
    H, F, rc, big = shape
    return X.inputs(X.graph(name), H, F, rc, big)


def _square(be, name, shape):
    key = (name, shape)
    if key not in _SQUARE:
        out = R.square_layer(be, name, _inputs(name, shape))
        for v in out.values():
            v.setflags(write=False)
        _SQUARE[key] = out
    return _SQUARE[key]


@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("part", range(4), ids=R.IDS)
@pytest.mark.parametrize("name", ("hub", "cora"))
def test_partitions_against_the_square_pair_and_float64(name, part, shape):
    be = backend.HipBackend()
    i = _inputs(name, shape)
    world, bounds = R.partitions(name)[part]
    got, parts = R.rect_layer(be, name, bounds, i)
    want = _square(be, name, shape)
    assert len(parts) == world
    for k in R.NAMES:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, name, R.IDS[part])
    g = X.graph(name)
    ref = X.exact_layer(g, i.aL, got["aR"], i.X, i.dY, i.heads)
    worst = X.check(f"gpu rect {name} {R.IDS[part]} {R.shape_id(shape)}", {k: got[k] for k in X.QUANTITIES}, ref, g)
    path = os.environ.get("GALA_GAT_EXACT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": f"{name}-{R.IDS[part]}-{R.shape_id(shape)}", "backend": "hip", **worst}) + "\n")


@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
def test_square_pair_is_pre_plus_gather(shape):
    """The old entry points give the bits of the forward, the pre-pass and the gather at self_col NULL."""
    be = backend.HipBackend()
    got = R.square_split(be, "hub", _inputs("hub", shape))
    want = _square(be, "hub", shape)
    for k in R.NAMES:
        assert np.array_equal(got[k], want[k]), k
