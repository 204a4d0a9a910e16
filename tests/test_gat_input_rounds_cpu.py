"""CPU: the graphs of the hub-chunk pre-pass past one round per wave, and the host twins on them.

k_gat_in_chunks (csrc/gat_input.hip) runs one wave per chunk on a grid capped at 4096 waves;
_rounds.round_hub_graph has more than 2 * 4096 chunks under the plan (64, 64).  This file
checks the graphs (check_round_hub_graph, from the plan's own arrays) and runs libgala_cpu.so's
twins (tests/test_gat_input_hub_cpu.py's cpu_layer_plan) against the oracle's float64-checked
REF layer on them at that file's tolerances, so the host results the kernels are compared with
in tests/test_gpu_gat_input_rounds.py are themselves shown good at this size.  Also the graph of
the k_gat_in_prep / k_gat_in_q test, and _rounds.dense_grad_plan against the library's own
workspace sizes.
"""
import numpy as np
import pytest

from gala import _abi, layout
from _rounds import (CHUNK_ROUND, ROUND_PLAN, check_prep_q_graph, check_round_hub_graph, dense_grad_plan,
                     prep_q_graph, round_hub_graph)
from test_gat_input_cpu import grad_close, layer_inputs, ref_on_own_logits
from test_gat_input_hub_cpu import check_twin_against_ref, cpu_layer_plan

SHAPES = [(100, 8, 32), (37, 4, 16)]
_CACHE = {}


def round_graphs(kind):
    """(g, gT, the orientation whose plan is the checked one: 0 g, 1 gT) for kind "sym", "dir"
    (the forward walks the checked graph's chunks) or "dirT" (the backward does); built and
    checked once."""
    if not _CACHE:
        s, d = round_hub_graph(True), round_hub_graph(False)
        _CACHE["nc"] = {"sym": check_round_hub_graph(s, True), "dir": check_round_hub_graph(d, False)}
        dT = layout.transpose(d)[0]
        _CACHE.update(sym=(s, s, 0), dir=(d, dT, 0), dirT=(dT, d, 1))
    return _CACHE[kind]


def n_hub_rows(kind):
    g = round_graphs(kind)
    return int((np.diff((g[1] if g[2] else g[0]).rowptr) > ROUND_PLAN[0]).sum())


def test_round_graphs_are_what_the_tests_rely_on():
    for kind in ("sym", "dir"):
        round_graphs(kind)
        assert _CACHE["nc"][kind] > 2 * CHUNK_ROUND
    check_prep_q_graph(prep_q_graph())


@pytest.mark.parametrize("kind", ["sym", "dir", "dirT"])
@pytest.mark.parametrize("fin,heads,D", SHAPES)
def test_twins_against_the_reference_past_one_round_of_chunks(fin, heads, D, kind):
    g, gT, side = round_graphs(kind)
    inp = layer_inputs(g.n_rows, fin, heads, D, seed=fin + heads)
    got = cpu_layer_plan(g, gT, ROUND_PLAN, *inp, heads, relu=True)
    assert got["hubs"][side] == n_hub_rows(kind) > 3000
    check_twin_against_ref(got, ref_on_own_logits(g, got, *inp, heads, relu=True))


def test_twin_spotlight_gradient_on_hub_columns():
    """dY zero off the hub rows: M and dW are the hub columns' aggregates alone (a lost chunk
    cannot hide under 1e-4 of another column's entries)."""
    g, gT, _ = round_graphs("sym")
    fin, heads, D = 100, 8, 32
    X, W, b, wL, bL, wR, bR, dY = layer_inputs(g.n_rows, fin, heads, D, seed=43)
    dY[np.diff(g.rowptr) <= ROUND_PLAN[0]] = 0
    got = cpu_layer_plan(g, gT, ROUND_PLAN, X, W, b, wL, bL, wR, bR, dY, heads)
    ref = ref_on_own_logits(g, got, X, W, b, wL, bL, wR, bR, dY, heads)
    check_twin_against_ref(got, ref)
    for k in ("dW", "db"):
        grad_close(got[k], ref[k], k)


@pytest.mark.parametrize("N,K,M", [(140000, 5, 2), (70000, 16, 3), (16500, 68, 180), (33000, 132, 540),
                                   (50000, 32, 47), (70001, 5, 2), (3000, 100, 180), (100000, 128, 128)])
def test_dense_grad_plan_mirrors_the_library(N, K, M):
    """_rounds.dense_grad_plan against gala_dense_grad_workspace, which sizes the workspace from
    plan_for's chunk count: sizeof(float) (P + runs(P)) (M K + M), the larger of the float4 and
    the scalar plan."""
    def floats(P):
        return (P + (1 if P <= 64 else -(-P // 64))) * (M * K + M)
    a, b = dense_grad_plan(N, K, M, False), dense_grad_plan(N, K, M, True)
    assert _abi.lib().gala_dense_grad_workspace(N, K, M) == 4 * max(floats(a["P"]), floats(b["P"]))
