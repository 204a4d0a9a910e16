"""GPU: the input-space GAT kernels (csrc/gat_input.hip) past one phase per workgroup.

k_gat_in_fwd / k_gat_in_bwd are persistent: a workgroup of 8 waves takes 8 rows per phase and
steps by the grid (at most 512 workgroups), so only past 4096 rows does a wave live through a
second phase -- the row walk's prefetch of the next phase's row (bounds, column window, the
row's own logits, first batch), the barrier guarding the LDS stash's reuse, the backward's
accumulators across phases, the -1 of a phase that does not exist.  tests/_graphs.py's
phase_graph (8205 rows, prescribed hand-offs between rows of 0, 1, 16, 17, 64, 65 edges, rows
at every batch and column-window edge, a 5-row last block) puts every one of those in a test
of a few seconds, for the walk (directed and symmetric) and T mode, against the oracle's
pass-by-pass REF layer (ref_on_own_logits) and against the same rows computed as first-phase
rows (a rotated row order: bit-identical per row).

Tolerances: Y, q, d_aL at the suite's 1e-4 (check_against_ref); the parameter gradients by
grad_close (1e-4 of the tensor's largest entry) and element-wise by grad_close_elementwise at
GRAD_C = 1e-5 of the element's own sum of absolute terms (measured and derived in
tests/test_gat_input_phases_cpu.py); T mode against the walk by the bounds of
tmode_against_walk, from the float32 format alone.
"""
import numpy as np
import pytest
import torch

import oracle as orc
from gala import _abi, layout, ops
from _graphs import PHASE_N, PHASE_STEP, check_phase_graph, phase_graph
from test_gat_input_cpu import layer_inputs, own_logits, ref_on_own_logits
from test_gat_input_phases_cpu import GRAD_C, grad_close_elementwise, grad_masses
from test_gpu_gat_input import E, TOL, check_against_ref, dev, mirror_op_against_the_chain  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(100, 8, 32), (37, 4, 16), (100, 3, 4), (64, 8, 8)]
U = 2.0 ** -24   # float32 unit roundoff
ROW_KEYS = ("Y", "Ym", "q", "sma", "daL")


class PhaseCase:
    """One phase_graph variant with its transposed pattern on the device and its row orders."""

    def __init__(self, symmetric):
        self.symmetric = symmetric
        self.g = phase_graph(symmetric)
        check_phase_graph(self.g, symmetric)
        self.gT = self.g if symmetric else layout.transpose(self.g)[0]
        self.deg = np.diff(self.g.rowptr)
        self.dg = ops.DeviceGraph.from_host(self.g, split=False)
        self.dgT = None if symmetric else ops.DeviceGraph.from_host(self.gT, split=False)
        n = self.g.n_rows
        ident = np.arange(n, dtype=np.int32)
        # name -> (order over g's rows, order over gT's rows); "rot1" / "rot2" make the rows of
        # the identity order's second / third phase first-phase rows
        self.orders = {"identity": (ident, ident),
                       "degree": (ops.degree_order(self.g.rowptr), ops.degree_order(self.gT.rowptr)),
                       "rot1": (np.roll(ident, -PHASE_STEP),) * 2,
                       "rot2": (np.roll(ident, -2 * PHASE_STEP),) * 2}


@pytest.fixture(scope="module")
def cases():
    return {False: PhaseCase(False), True: PhaseCase(True)}


def run_layer(case, inp, heads, order="identity", relu=False, tmode=False, **kw):
    """test_gpu_gat_input.gpu_layer with an order of its own for the transposed pattern; Ym,
    sma, M and (on the device) T kept."""
    X, W, b, wL, bL, wR, bR, dY = inp
    o, ot = (dev(a) for a in case.orders[order])
    out = ops.gat_input_layer(case.dg, dev(X), dev(W), dev(b), dev(wL), dev(bL), dev(wR), dev(bR), heads, dY=dev(dY),
                              gT=case.dgT, relu=relu, order=o, order_t=ot, tmode=tmode, **kw)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "T"}
    got["T"] = out["T"]
    return got


def phase_of(case, order):
    """Phase number of every row under a row order: (position // 8) // 512."""
    o = case.orders[order][0]
    ph = np.empty(len(o), np.int64)
    ph[o] = (np.arange(len(o)) // 8) // 512
    return ph


def localise(case, order, bad_rows, worst, what):
    """Failure text that tells a first-phase error from a hand-off error."""
    ph = phase_of(case, order)
    o = case.orders[order][0]
    pos = np.empty(len(o), np.int64)
    pos[o] = np.arange(len(o))
    per = {int(k): int((ph[bad_rows] == k).sum()) for k in np.unique(ph[bad_rows])}
    prev = int(o[pos[worst] - PHASE_STEP]) if pos[worst] >= PHASE_STEP else None
    kind = ("a first-phase row: the walk itself" if ph[worst] == 0 else
            f"a row handed off to by row {prev} (degree {int(case.deg[prev])}): the next-row prefetch / stash reuse")
    return (f"{what}: worst row {int(worst)}, degree {int(case.deg[worst])}, phase {int(ph[worst])} ({kind}); "
            f"rows over the bound per phase {per} (order {order})")


def check_rows_against_ref(case, order, got, ref):
    """check_against_ref's bounds on Y, q, d_aL per row, with the worst row located."""
    for k, tol in (("Y", TOL), ("q", dict(atol=0.0, rtol=1e-4)), ("daL", TOL)):
        a, w = got[k].astype(np.float64), ref[k].astype(np.float64)
        over = (np.abs(a - w) - (tol["atol"] + tol["rtol"] * np.abs(w))).reshape(len(a), -1).max(1)
        over = np.where(np.isnan(over), np.inf, over)
        if (over > 0).any():
            raise AssertionError(localise(case, order, np.flatnonzero(over > 0), int(np.argmax(over)),
                                          f"{k} against the reference chain"))


def check_layer(case, inp, heads, order, relu, tmode):
    X, W, b, wL, bL, wR, bR, dY = inp
    got = run_layer(case, inp, heads, order, relu, tmode)
    ref = ref_on_own_logits(case.g, got, X, W, b, wL, bL, wR, bR, dY, heads, relu=relu)
    check_rows_against_ref(case, order, got, ref)
    check_against_ref(got, ref)
    empty = case.deg == 0
    assert empty.any() and np.all(got["Y"][empty] == 0) and np.all(got["q"][empty] == np.float32(1e12))
    mass = grad_masses(ref, X, heads)
    for k in ("dW", "db", "dwL", "dbL", "dwR", "dbR"):
        grad_close_elementwise(got[k], ref[k], mass[k], GRAD_C, f"{k} order={order} relu={relu} tmode={tmode} ")
    return got, ref


def inputs(fin, heads, D):
    return layer_inputs(PHASE_N, fin, heads, D, seed=fin + heads)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("order", ["identity", "degree"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["directed", "symmetric"])
@pytest.mark.parametrize("fin,heads,D", SHAPES)
def test_walk_past_one_phase_against_the_reference_chain(cases, fin, heads, D, symmetric, order, relu):
    """gala_gat_in_fwd_f32 + gala_gat_in_bwd_f32 (the walk: k_gat_in_fwd<false>,
    k_gat_in_bwd<DW, false>) on 8205 rows; the directed graph's backward walks the transposed
    pattern in an order of its own."""
    check_layer(cases[symmetric], inputs(fin, heads, D), heads, order, relu, tmode=False)


def tmode_against_walk(case, order, gt, gw, inp, heads, relu):
    """T mode against the walk on the same inputs and order.  tools/gat_in_tmode_ab.py reports
    their largest differences and claims no bit-identity: T mode's q is the sequential row sum
    (k_gat_in_q), the walk's the MFMA-ordered one.  Everything else the two forwards compute
    is the same arithmetic, so with u = 2^-24 and, per row, d = (2 (deg - 1) + 6) u (two
    float32 sums of the same deg positive terms, each within (deg - 1) u; the 1e-12 added, the
    reciprocal and the product by q once each per mode):
      q, and Y, Ym, sma = fl(q * .): relative difference <= d per element (empty rows: equal);
      d_aL = (sum dY Ym - (sum dY Y + 1e-12) sma) + 1e-12: inputs moved by d, two float32
        evaluations of D-term dots, so <= (2.01 d + 2 (D + 3) u) (sum |dY Ym| + sum |dY Y| |sma|);
      M = sum_r dX[r]^T Xext[r] with alpha = fl(p q[r]): <= 1.01 (d[r] sum_e alpha_e |dY[c_e]|)^T
        |Xext| for the moved q, plus 2 GRAD_C of the sum of absolute terms for the two float32
        accumulations (GRAD_C per accumulation: tests/test_gat_input_phases_cpu.py)."""
    X, W, b, wL, bL, wR, bR, dY = inp
    n, F = dY.shape
    D = F // heads
    d = ((2 * np.maximum(case.deg - 1, 0) + 6) * U).astype(np.float64)
    for k in ("q", "Y", "Ym", "sma"):
        a, w = gt[k].astype(np.float64), gw[k].astype(np.float64)
        over = (np.abs(a - w) - d[:, None] * np.abs(w)).max(1)
        assert not (over > 0).any(), localise(case, order, np.flatnonzero(over > 0), int(np.argmax(over)),
                                              f"T mode's {k} against the walk's")
    assert np.array_equal(gt["q"][case.deg == 0], gw["q"][case.deg == 0])
    dym = np.where(gw["Y"] > 0, dY, 0).astype(np.float64) if relu else dY.astype(np.float64)
    B = (np.abs(dym * gw["Ym"]).reshape(n, heads, D).sum(2)
         + np.abs(dym * gw["Y"]).reshape(n, heads, D).sum(2) * np.abs(gw["sma"]))
    bound = (2.01 * d[:, None] + 2 * (D + 3) * U) * B + 1e-11
    over = (np.abs(gt["daL"].astype(np.float64) - gw["daL"]) - bound).max(1)
    assert not (over > 0).any(), localise(case, order, np.flatnonzero(over > 0), int(np.argmax(over)),
                                          "T mode's d_aL against the walk's")
    # the sums of absolute terms of M: the REF backward on |dY| (alpha >= 0)
    aL, aR = own_logits(gt["xext"], heads)
    ab = orc.gat_input_layer_ref(case.g.rowptr, case.g.col, X, W, b, wL, bL, wR, bR,
                                 np.abs(dym).astype(np.float32), heads, aL=aL, aR=aR)
    xe = np.abs(np.concatenate([X, np.ones((n, 1), np.float32)], 1).astype(np.float64))
    dxa = np.abs(ab["dX"].astype(np.float64))
    bound = (1.01 * ((d[:, None] * dxa).T @ xe) + 2 * GRAD_C * (dxa.T @ xe)).reshape(heads, D, -1) + 1e-6
    over = np.abs(gt["M"].astype(np.float64) - gw["M"]) - bound
    i = np.unravel_index(np.argmax(over), over.shape)
    assert over[i] <= 0, f"T mode's M{list(i)} against the walk's: {gt['M'][i]} vs {gw['M'][i]}, bound {bound[i]:.3g}"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("order", ["identity", "degree"])
@pytest.mark.parametrize("fin,heads,D", SHAPES)
def test_t_mode_past_one_phase_against_the_reference_chain_and_the_walk(cases, fin, heads, D, order, relu):
    """gala_gat_in_fwd_t_f32 + gala_gat_in_bwd_t_f32 (k_gat_in_fwd<true>, k_gat_in_bwd<DW, true>)
    on the symmetric 8205 rows: against the reference chain, and against the walk on the same
    inputs and order (tmode_against_walk)."""
    case, inp = cases[True], inputs(fin, heads, D)
    gt, ref = check_layer(case, inp, heads, order, relu, tmode=True)
    assert gt["T"] is not None
    gw = run_layer(case, inp, heads, order, relu, tmode=False)
    tmode_against_walk(case, order, gt, gw, inp, heads, relu)


@pytest.mark.parametrize("mode", ["walk-directed", "walk-symmetric", "tmode"])
@pytest.mark.parametrize("fin,heads,D", SHAPES)
def test_rows_of_later_phases_equal_the_same_rows_as_first_phase_rows(cases, fin, heads, D, mode):
    """A row's own sums do not depend on the row order, so every output row (Y, Ym, q, sma,
    d_aL; T mode: its T tiles) is bit-identical between the identity order, where rows >= 4096
    are reached through a hand-off (rows >= 8192 through two), and the orders rotated by 4096
    and 8192, where they are the workgroups' first rows (cursor_start, no prefetch).  A
    difference names the row, its degree and its phase in the identity order."""
    case = cases[mode != "walk-directed"]
    inp, tmode = inputs(fin, heads, D), mode == "tmode"
    base = run_layer(case, inp, heads, "identity", relu=True, tmode=tmode)
    ph = phase_of(case, "identity")
    assert (ph >= 1).sum() == PHASE_N - PHASE_STEP and (ph == 2).sum() == PHASE_N - 2 * PHASE_STEP
    for rot, first in (("rot1", ph == 1), ("rot2", ph == 2)):
        assert (phase_of(case, rot)[first] == 0).all()
        got = run_layer(case, inp, heads, rot, relu=True, tmode=tmode)
        for k in ROW_KEYS:
            diff = (got[k] != base[k]).reshape(PHASE_N, -1).any(1)
            assert not diff.any(), localise(case, "identity", np.flatnonzero(diff), int(np.flatnonzero(diff)[0]),
                                            f"{k} differs between the identity order and {rot}")
        if tmode:
            diff = (got["T"] != base["T"]).any(1).cpu().numpy()
            assert not diff.any(), localise(case, "identity", np.flatnonzero(diff), int(np.flatnonzero(diff)[0]),
                                            f"T differs between the identity order and {rot}")


@pytest.mark.parametrize("symmetric", [False, True], ids=["directed-walk", "symmetric-tmode"])
def test_mirror_op_equals_the_three_op_chain_past_one_phase(E, symmetric):
    """test_mirror_op_equals_the_three_op_chain's body on phase_graph: gat_input_layer_apply
    runs T mode on the symmetric variant (its pattern equals its transpose: check_phase_graph)
    and, on the directed one, the forward walk and the backward's walk over the transposed
    pattern, both at more than one phase per workgroup.  The chain's ReLU takes the op's own
    mask (mirror_op_against_the_chain: with torch.relu on the chain's own output, 2.1 M outputs
    at ~1e-7 apart put a few on opposite sides of 0, and the directed variant's dW then misses
    1e-4 by one edge's term, 0.057 against 0.005); Y itself is held to 1e-4 either way."""
    g = phase_graph(symmetric)
    check_phase_graph(g, symmetric)
    mirror_op_against_the_chain(E, g, pin_relu_mask=True)
    E.slots_clear()


def padded(a, pad, fill):
    """a as the leading columns of a buffer `pad` columns wider, the rest holding `fill`."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, device="cuda", dtype=torch.float32)
    buf[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return buf, buf[:, :a.shape[1]]


@pytest.mark.parametrize("mode", ["walk-directed", "tmode"])
def test_leading_dimensions_of_views_into_wider_buffers(cases, mode):
    """ldxin, ldw and ldy as the kernels take them: X, W, dY column views of wider buffers whose
    padding holds NaN, Y and Ym column views whose padding holds 7.0 (ldy = F + 4: a multiple
    of 4 floats, rows 16-byte aligned).  Every output is bit-identical to the packed call's and
    the output padding is untouched."""
    fin, heads, D = 37, 4, 16
    F = heads * D
    case, tmode = cases[mode == "tmode"], mode == "tmode"
    inp = inputs(fin, heads, D)
    X, W, b, wL, bL, wR, bR, dY = inp
    base = run_layer(case, inp, heads, "identity", relu=True, tmode=tmode)
    nan = float("nan")
    (xb, xv), (wb, wv), (db_, dv) = padded(X, 3, nan), padded(W, 5, nan), padded(dY, 4, nan)
    (yb, yv), (ymb, ymv) = (padded(np.zeros((PHASE_N, F), np.float32), 4, 7.0) for _ in range(2))
    assert xv.stride(0) == fin + 3 and wv.stride(0) == fin + 5 and yv.stride(0) == F + 4 and dv.stride(0) == F + 4
    o, ot = (dev(a) for a in case.orders["identity"])
    out = ops.gat_input_layer(case.dg, xv, wv, dev(b), dev(wL), dev(bL), dev(wR), dev(bR), heads, dY=dv, gT=case.dgT,
                              relu=True, order=o, order_t=ot, tmode=tmode, Y=yv, Ym=ymv)
    torch.cuda.synchronize()
    assert out["Y"].data_ptr() == yb.data_ptr() and out["Ym"].data_ptr() == ymb.data_ptr()
    for k in ROW_KEYS + ("M", "dW", "db", "dwL", "dbL"):
        np.testing.assert_array_equal(out[k].cpu().numpy(), base[k], err_msg=k)
    assert (yb[:, F:] == 7.0).all() and (ymb[:, F:] == 7.0).all()
    assert torch.isnan(xb[:, fin:]).all() and torch.isnan(wb[:, fin:]).all() and torch.isnan(db_[:, F:]).all()


def test_backward_refuses_a_row_stride_that_is_no_multiple_of_four(cases):
    """The backward loads dY, Y, Ym rows as float4: ldy % 4 != 0 is GALA_ERR_INVALID_ARG, in both
    formulations, before any launch."""
    fin, heads, D = 37, 4, 16
    F = heads * D
    case = cases[True]
    bufs = [torch.zeros(PHASE_N, F + 3, device="cuda") for _ in range(3)]
    dY, Y, Ym = (t[:, :F] for t in bufs)
    xext = torch.zeros(PHASE_N, 128, device="cuda")
    sma = torch.zeros(PHASE_N, heads, device="cuda")
    for T in (None, torch.zeros(PHASE_N, 896, device="cuda")):
        with pytest.raises(_abi.GalaError) as ei:
            ops.gat_in_bwd(case.dg, xext, dY, Y, Ym, sma, heads, fin, T=T)
        assert ei.value.status == _abi.GALA_ERR_INVALID_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("symmetric", [False, True], ids=["directed-walk", "symmetric-tmode"])
def test_mirror_backward_takes_a_grad_at_an_unaligned_storage_offset(E, symmetric):
    """A contiguous grad 4 bytes into its storage (a view of a larger buffer) through
    gat_input_layer_apply's backward, whose kernels read dY rows as float4: the gradients are
    bit-identical to those from an aligned copy."""
    g = phase_graph(symmetric)
    fin, H, D = 37, 4, 16
    n, F = g.n_rows, H * D
    E.slots_clear()
    off, cols = dev(g.rowptr), dev(g.col)
    vals = torch.ones(g.nnz, device="cuda")
    E.slots_push(off, cols, vals, None, 1, False)
    E.slots_push(off, cols, vals, None, 1, False)
    X, W, b, wL, bL, wR, bR, dY = layer_inputs(n, fin, H, D, seed=9)
    params = [dev(a).requires_grad_() for a in (W, b, wL.reshape(1, -1), bL, wR.reshape(1, -1), bR)]
    x = dev(X)
    assert E.gat_input_layer_eligible(x, params[0], 0, H, 0)
    buf = torch.zeros(n * F + 8, device="cuda")
    buf[1:1 + n * F] = dev(dY).reshape(-1)
    shifted = buf[1:1 + n * F].view(n, F)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and dev(dY).data_ptr() % 16 == 0
    grads = []
    for grad in (dev(dY), shifted):
        for p in params:
            p.grad = None
        Y = E.gat_input_layer_apply(x, *params, 0, 0.2, 0, True)
        Y.backward(grad)
        grads.append([p.grad.cpu().numpy() for p in params])
    E.slots_clear()
    for name, a, w in zip(("W", "b", "wL", "bL", "wR", "bR"), grads[1], grads[0]):
        np.testing.assert_array_equal(a, w, err_msg=name)


def test_t_mode_refuses_a_directed_graph(cases):
    """T mode forms the backward's aggregates over g itself: without the transposed pattern it
    needs a symmetric g.  The directed phase_graph is refused with ValueError before anything
    is launched (no tensor argument is looked at: all None here); the symmetric one passes the
    same check."""
    with pytest.raises(ValueError, match="symmetric"):
        ops.gat_input_layer(cases[False].dg, None, None, None, None, None, None, None, 4, tmode=True)
    assert ops.pattern_is_symmetric(cases[True].dg) and not ops.pattern_is_symmetric(cases[False].dg)
