"""A FIXED GAT layer through the operator mirror (gat_aggregate_apply / gat_aggregate_ffn_apply)
with GALA_GAT_EXACT_STATS on (the exact statistics pair) and off (the alpha-storing path):
outputs and gradients against the float64 layer, peak memory, and the cases that keep the old
path bit for bit."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import _gat_exact_ref as X
from gala import layout

pytestmark = pytest.mark.gpu
ENV = "GALA_GAT_EXACT_STATS"


@pytest.fixture(scope="module")
def E():
    import gala
    return gala.torch_ext()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _push(E, g, bw=None, perm=None):
    """Slot 0 = g, slot 1 = its transpose with the edge permutation (a FIXED program's slots)."""
    E.slots_clear()
    E.slots_push(_dev(g.rowptr), _dev(g.col), torch.ones(g.nnz, device="cuda"), None, 1, False)
    if bw is None:
        bw, perm = layout.transpose(g)
    E.slots_push(_dev(bw.rowptr), _dev(bw.col), torch.ones(bw.nnz, device="cuda"), None, 1, False)
    E.slots_set_transpose_perm(1, _dev(perm))


def _layer(E, i, H, exact, ffn=False, measure=False):
    """One forward + backward; (Y, grads..., peak bytes above the inputs and outputs)."""
    os.environ[ENV] = "1" if exact else "0"
    try:
        aL, Xd = _dev(i.aL).requires_grad_(), _dev(i.X).requires_grad_()
        w = _dev(i.dY)
        if ffn:
            wR, bR = _dev(i.wR.reshape(1, -1)).requires_grad_(), _dev(i.bR).requires_grad_()
            ins = [aL, Xd, wR, bR]
        else:
            aR = _dev(i.aR).requires_grad_()
            ins = [aL, aR, Xd]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        if ffn:
            Y = E.gat_aggregate_ffn_apply(aL, Xd, wR, bR, 0, X.SLOPE, 1)
        else:
            Y = E.gat_aggregate_apply(aL, aR, Xd, 0, X.SLOPE, 1)
        Y.backward(w)
        torch.cuda.synchronize()
        outs = [Y.detach()] + [t.grad for t in ins]
        peak = torch.cuda.max_memory_allocated() - base - sum(o.numel() * 4 for o in outs)
        return [o.cpu().numpy() for o in outs], peak
    finally:
        os.environ.pop(ENV, None)


_DENSE = {}


def _dense_graph():
    """2 000 rows, about 1 100 edges per row after symmetrising: E * H * 4 bytes dwarf n * F * 4."""
    if not _DENSE:
        _DENSE["g"] = X.symmetrise(X.G.long_row_graph())
    return _DENSE["g"]


def test_fixed_layer_on_and_off_and_peak_memory(E):
    """aR given, 8 heads x 8: both paths within the float64 bounds; the new path's peak allocation
    above its inputs and outputs is below E * H * 4 bytes (one alpha), which the old path, that
    stores alpha, its transpose and dz, cannot meet."""
    g = _dense_graph()
    H, F = 8, 64
    i = X.inputs(g, H, F, False, False)
    _push(E, g)
    on, peak_on = _layer(E, i, H, True)
    off, peak_off = _layer(E, i, H, False)
    ref = X.exact_layer(g, i.aL, i.aR, i.X, i.dY, H)
    for tag, o in (("on", on), ("off", off)):
        got = dict(Y=o[0], daL=o[1], daR=o[2], dX=o[3])
        X.check(f"mirror {tag}", {k: v.reshape(g.n_rows, -1) for k, v in got.items()}, ref, g, chunk=None)
    eh4 = g.nnz * H * 4
    print(f"peak above inputs and outputs: exact {peak_on} B, alpha-storing {peak_off} B, E*H*4 = {eh4} B")
    assert peak_on < eh4, (peak_on, eh4)
    assert peak_off >= eh4, (peak_off, eh4)        # the switch does switch


def test_fixed_ffn_layer_on_and_off(E):
    """The DSL's layer (aR = Linear(X) recomputed in the kernels), 8 heads x 32 on the graph with
    hub and empty rows: Y and every gradient agree between the two paths within the sum of
    their float64 bounds; d_aR reaches the Linear distinct from d_aL."""
    g = X.graph("hub")
    H, F = 8, 256
    i = X.inputs(g, H, F, True, False)
    _push(E, g)
    on, _ = _layer(E, i, H, True, ffn=True)
    off, _ = _layer(E, i, H, False, ffn=True)
    ar64, _ = X.source_logits(i.X, i.wR, i.bR, H)
    ref = X.exact_layer(g, i.aL, ar64.astype(np.float32), i.X, i.dY, H)
    X.check("mirror ffn Y", dict(Y=on[0]), ref, g)
    X.check("mirror ffn daL", dict(daL=on[1].reshape(g.n_rows, -1)), ref, g)
    # dX = the layer's dX + d_aR wR, dW = d_aR^T X, db = sum d_aR: float64 from the reference's parts
    D = F // H
    wR = i.wR.astype(np.float64)
    dX64 = ref.dX + np.repeat(ref.daR, D, axis=1) * wR[None, :]
    dXm = ref.dX_mass + np.repeat(ref.daR_mass, D, axis=1) * np.abs(wR)[None, :]
    x64 = i.X.astype(np.float64)
    dW64 = (np.repeat(ref.daR, D, axis=1) * x64).sum(0)
    dWm = (np.repeat(ref.daR_mass, D, axis=1) * np.abs(x64)).sum(0)
    for tag, o in (("on", on), ("off", off)):
        X.E.assert_bounded(f"ffn {tag} dX", o[2], dX64, dXm, X.C["dX"], g=g, per="row", record=False)
        X.E.assert_bounded(f"ffn {tag} dW", o[3].ravel(), dW64, dWm, X.C["daR"], record=False)
        X.E.assert_bounded(f"ffn {tag} db", o[4].ravel(), ref.daR.sum(0), ref.daR_mass.sum(0), X.C["daR"], record=False)
    assert np.abs(ref.daR - ref.daL).max() > 1e-3


def _both(E, i, H, ffn=False):
    on, _ = _layer(E, i, H, True, ffn=ffn)
    off, _ = _layer(E, i, H, False, ffn=ffn)
    return on, off


def test_cases_that_keep_the_old_path(E):
    """A directed pattern and a slot 2li+1 that is not the forward's pattern tensor for tensor:
    each bit-identical to GALA_GAT_EXACT_STATS=0.  A shape the statistics pair refuses: no such
    shape runs on the old path either, so the layer raises the same error both ways."""
    # directed
    d = X.G.with_empty_rows()
    _push(E, d)
    on, off = _both(E, X.inputs(d, 4, 32, False, False), 4)
    assert all(np.array_equal(a, b) for a, b in zip(on, off))
    # the same symmetric matrix in slot 1, two columns of one row stored in the other order
    g = X.graph("cora")
    t, perm = layout.transpose(g)
    r = int(np.flatnonzero(np.diff(g.rowptr) >= 2)[0])
    e = int(g.rowptr[r])
    col, perm = t.col.copy(), perm.copy()
    col[[e, e + 1]], perm[[e, e + 1]] = col[[e + 1, e]], perm[[e + 1, e]]
    bw = layout.HostGraph(t.n_rows, t.n_cols, t.rowptr, col, None)
    _push(E, g, bw, perm)
    i = X.inputs(g, 4, 32, False, False)
    on, off = _both(E, i, 4)
    assert all(np.array_equal(a, b) for a, b in zip(on, off))
    _push(E, g)                                   # (with its own transpose the new path runs: other bits)
    on2, _ = _layer(E, i, 4, True)
    assert not all(np.array_equal(a, b) for a, b in zip(on2, off))
    # 2 heads x 6 (three float2 lanes per head) is refused by the pair -- and by the kernels of
    # the alpha-storing backward, which refuse every shape the pair refuses (several heads need
    # a power of two of lanes per head there too): the layer fails the same way on and off
    j = X.inputs(g, 2, 12, False, False)
    for exact in (True, False):
        with pytest.raises(RuntimeError, match="GALA_ERR_UNSUPPORTED"):
            _layer(E, j, 2, exact)


def test_compiled_two_layer_fixed_program(tmp_path):
    """tests/dsl/gat_exact.txt (two layers, gat_heads(8), gat_fixed_gradients(true)) compiled by
    galac: its run on the GPU against the float64 semantics of its IR, gradients included."""
    from _dsl_check import PROGS, check_against_ir, run_prog
    assert "gat_exact" in PROGS, "run tools/build_dsl_progs.py (build()) first"
    _, d = run_prog("gat_exact", tmp_path, "--iters", "6")
    check_against_ir("gat_exact", d)
