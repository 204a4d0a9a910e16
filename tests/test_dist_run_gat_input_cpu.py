"""CPU (host backend, gloo): a GAT program's first layer in input space under gala.dist_run.

tests/dsl/gat_input.txt is config 3's layer shape shrunk (20 input features, 4 heads of 8, ReLU,
then a one-head layer of the classes): layer 1 meets plan_input_layers and input_layer_eligible
and runs as _GatInputLayer over gala.dist.HaloGatInput, layer 2 (its input is no dataset feature)
stays on the row-statistics pair (HaloGat).  Graphs: --synthetic (2708 rows) and an R-MAT graph
with a row past the hub-row threshold (a Matrix Market file).

* the summary's gat_layers names the layer each node ran, and its byte counts are the layer's;
* GALA_GAT_INPUT=0 runs the parent's three ops: every entry "stats";
* input space against the three ops at one world size, and worlds 2 / 3 against world 1: the
  tolerance tests/test_dist_run_cpu.py applies between layouts of a GAT program (PRED_TOL,
  LOSS_TOL below, copied from test_dist_run_gat_ranks_match_one_rank), on the first loss, the
  loss curve, the layer-1 rows and every parameter after one Adam step; across world sizes
  the layer-1 rows and the predictions are bit-identical;
* eval forwards (torch.no_grad()) run no q exchange and equal the training forward bit for bit;
* every condition of input_layer_eligible has a negative case.
"""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import _ir_ref as ref
from _dist_check import check_dist_dump
from test_dist_run_cpu import _ir, _run

PRED_TOL = dict(rtol=1e-4, atol=1e-5)      # tests/test_dist_run_cpu.py, GAT program between layouts
LOSS_TOL = dict(rtol=1e-4, atol=1e-6)
PROG = "gat_input.txt"
HEADS, L1, L2 = 4, 7, 15                   # the program's heads and its GAT nodes' values
ITERS = 4


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():       # None: unset
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def write_mtx(g, path):
    """The host graph's pattern as a Matrix Market `general` file (dist_run --data FILE.mtx)."""
    rows = np.repeat(np.arange(g.n_rows), np.diff(g.rowptr.astype(np.int64)))
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate pattern general\n{g.n_rows} {g.n_cols} {g.nnz}\n")
        np.savetxt(f, np.stack([rows + 1, g.col.astype(np.int64) + 1], 1), fmt="%d")


def rmat_hub_graph():
    """R-MAT, 4096 rows: symmetric, and its longest row exceeds the graph's hub-row threshold."""
    from gala import layout
    g = layout.gen_graph("rmat", 4096, 40000, seed=11)
    deg = np.diff(g.rowptr.astype(np.int64))
    assert deg.max() > layout.split_threshold(g.n_rows, g.nnz)
    t = layout.transpose(g)[0]
    assert np.array_equal(t.rowptr, g.rowptr) and np.array_equal(t.col, g.col)
    return g


class Runs:
    """gala.dist_run launches of this module, each run once (keyed by its arguments)."""

    def __init__(self, tmp, run=_run):
        self.tmp, self.run, self.done, self.irs = tmp, run, {}, {}

    def ir(self, prog=PROG, edit=None):
        """The program's IR; edit (old, new): a variant of the DSL text."""
        key = (prog, edit)
        if key not in self.irs:
            d = self.tmp / f"ir{len(self.irs)}"
            d.mkdir()
            if edit is None:
                self.irs[key] = _ir(prog, d)
            else:
                here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dsl")
                text = open(os.path.join(here, prog)).read()
                assert edit[0] in text
                (d / "variant.txt").write_text(text.replace(*edit))
                self.irs[key] = _ir(str(d / "variant.txt"), d)
        return self.irs[key]

    def rmat(self):
        p = self.tmp / "rmat.mtx"
        if not p.exists():
            write_mtx(rmat_hub_graph(), p)
        return ("--data", str(p))

    def __call__(self, world=1, switch=None, extra=(), iters=ITERS, prog=PROG, edit=None, env=None):
        key = (world, switch, tuple(extra), iters, prog, edit, tuple(sorted((env or {}).items())))
        if key not in self.done:
            with _env(GALA_GAT_INPUT=switch, **(env or {})):
                self.done[key] = self.run(self.ir(prog, edit), self.tmp, world, f"r{len(self.done)}", iters=iters,
                                          extra=tuple(extra))
        return self.done[key]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("gat_input"))


def kinds(summary):
    return [(e["node"], e["kind"]) for e in summary["gat_layers"]]


def check_pair(a, b, bitwise_rows=False):
    """Two dumps of one program on one graph: item 3's tolerance on the first loss, the curve, the
    layer-1 rows, the predictions and every parameter after one Adam step."""
    np.testing.assert_allclose(a["losses"][0], b["losses"][0], **LOSS_TOL)
    np.testing.assert_allclose(a["losses"], b["losses"], **LOSS_TOL)
    if bitwise_rows:
        np.testing.assert_array_equal(a[f"gat_out:{L1}"], b[f"gat_out:{L1}"])
        np.testing.assert_array_equal(a["prediction"], b["prediction"])
    else:
        # (the input-space layer's rows carry the folded ReLU; the three ops' are taken before it)
        np.testing.assert_allclose(np.maximum(a[f"gat_out:{L1}"], 0), np.maximum(b[f"gat_out:{L1}"], 0), **PRED_TOL)
        np.testing.assert_allclose(a["prediction"], b["prediction"], **PRED_TOL)
    steps = [k for k in a if k.startswith("step1:")]
    assert len(steps) == 6 * 2 and sorted(steps) == sorted(k for k in b if k.startswith("step1:"))
    for k in steps:
        np.testing.assert_allclose(a[k], b[k], err_msg=k, **PRED_TOL)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_run_takes_the_input_space_layer(runs, world):
    """gat_layers: layer 1 "input", layer 2 "stats"; the host backend has the walk only; at world
    > 1 the input layer moves 4 H bytes of q per halo row of rank 0 and step, and fetched that
    rank's halo input rows once."""
    d, s = runs(world)
    assert kinds(s) == [(L1, "input"), (L2, "stats")]
    e1, e2 = s["gat_layers"]
    assert e1["tmode"] is False and e2["tmode"] is False and e2["setup_bytes"] == 0
    if world == 1:
        assert e1["halo_bytes_per_step"] == 0 and e1["setup_bytes"] == 0 and s["q_exchanges"] == 0
        return
    from gala import dist as gdist
    from gala import layout
    g = layout.HostGraph(len(d["rowptr"]) - 1, len(d["rowptr"]) - 1, d["rowptr"], d["col"])
    part = gdist.partition_graph(g, 0, world)
    assert part.n_halo_rows > 0 and e1["halo_bytes_per_step"] == 4 * HEADS * part.n_halo_rows
    assert e1["setup_bytes"] == part.halo_bytes(20)
    assert e2["halo_bytes_per_step"] == part.halo_bytes(2 * 7 + 1)
    assert s["q_exchanges"] == ITERS          # one per training forward
    assert s["loss_last"] < s["loss_first"]


def test_one_rank_matches_ir_semantics(runs):
    """World 1 in input space against the float64 executor of the IR's three nodes: forward,
    loss and the first epoch's weight gradients."""
    d, _ = runs(1)
    check_dist_dump(runs.ir(), d)


@pytest.mark.parametrize("world", [1, 2])
def test_switch_falls_back_to_the_three_ops(runs, world):
    """GALA_GAT_INPUT=0: every entry "stats" -- HaloGat with F + H floats per halo row forward and F
    backward -- and the run is the three-op path's: a second launch repeats it exactly."""
    d, s = runs(world, switch="0")
    assert kinds(s) == [(L1, "stats"), (L2, "stats")] and s["q_exchanges"] == 0
    assert all(e["setup_bytes"] == 0 and not e["tmode"] for e in s["gat_layers"])
    if world > 1:
        e1, e2 = s["gat_layers"]
        assert e1["halo_bytes_per_step"] * (2 * 7 + 1) == e2["halo_bytes_per_step"] * (2 * 32 + HEADS) > 0
    d2, s2 = runs(world, switch="0", extra=("--seed", "3"))     # the default seed, a second launch
    np.testing.assert_array_equal(d2["losses"], d["losses"])
    np.testing.assert_array_equal(d2["prediction"], d["prediction"])


@pytest.mark.parametrize("world", [1, 2, 3])
def test_input_space_matches_the_three_ops(runs, world):
    check_pair(runs(world)[0], runs(world, switch="0")[0])


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_match_one_rank_bit_for_bit(runs, world):
    """All input space: the layer-1 rows (and with HaloGat's layer 2 the predictions) of N ranks
    are bit-identical to one rank; losses and stepped parameters within the cross-rank sums'
    rounding."""
    check_pair(runs(world)[0], runs(1)[0], bitwise_rows=True)


@pytest.mark.parametrize("world", [1, 2])
def test_rmat_hub_row_graph(runs, world):
    """The R-MAT graph (a row past the hub-row threshold): input space, against the three ops,
    and two ranks bit-identical to one."""
    d, s = runs(world, extra=runs.rmat())
    assert kinds(s) == [(L1, "input"), (L2, "stats")] and s["vertices"] == 4096
    check_pair(d, runs(world, switch="0", extra=runs.rmat())[0])
    if world > 1:
        check_pair(d, runs(1, extra=runs.rmat())[0], bitwise_rows=True)


@pytest.mark.parametrize("world", [1, 2])
def test_eval_forwards_run_no_exchange(runs, world):
    """--eval: a no_grad forward before the first and after the last epoch.  The input layer
    runs HaloGatInput.forward: no q exchange (the layer's counter, and the message counters show
    only layer 2's two gathers per forward), and the first eval forward equals the first
    training forward -- the same weights -- bit for bit."""
    d, s = runs(world, extra=("--eval",))
    ev = s["eval"]
    assert ev["forwards"] == 2 and ev["q_exchanges"] == 0 and s["q_exchanges"] == (ITERS if world > 1 else 0)
    np.testing.assert_array_equal(d["eval_prediction"], d["prediction"])
    np.testing.assert_array_equal(d["prediction"], runs(world)[0]["prediction"])
    if world == 1:
        assert ev["messages"] == {}
    else:      # HaloGat (layer 2): the X rows, then the recomputed source logits; one peer
        kind = "p2p" if s["halo"] == "p2p" else "all_gather"
        assert ev["messages"] == {kind: 2 * ev["forwards"]}
        _, s0 = runs(world, switch="0", extra=("--eval",))
        assert s0["eval"]["messages"] == {kind: 4 * ev["forwards"]}


# ---- negative cases: one per condition of input_layer_eligible ---------------------------------
class _Part:
    chunks = 1

    def own_offset(self):
        return 0


def _eligible(ir, layout_mode="halo", part=None, symmetric=True):
    from gala import dist_run
    plan = dist_run.plan_input_layers(ir)
    nd = [n for n in ir["nodes"] if n["op"] == "GAT_AGGREGATE"]
    return [dist_run.input_layer_eligible(ir, n, plan, layout_mode, part or _Part(), symmetric) for n in nd]


@pytest.fixture(scope="module")
def ir(runs):
    return ref.load_ir(str(runs.ir()))["post"]


def test_plan_matches_the_first_layer_only(ir):
    from gala import dist_run
    assert dist_run.plan_input_layers(ir) == {L1: {"ffn": 1, "attn": 2, "relu": 8}}
    assert _eligible(ir) == [True, False]


def _edit(ir, fn):
    c = json.loads(json.dumps(ir))
    fn(c)
    return c


def _w(c, name):
    return next(w for w in c["weights"] if w["name"] == name)


@pytest.mark.parametrize("name,fn", [
    ("directed", lambda c: c["sched"].update(undirected=0)),
    ("fixed", lambda c: c["sched"].update(gat_mode=1)),
    ("ksample", lambda c: c["sched"].update(kernel_sample=5)),
    ("fin=H*D", lambda c: _w(c, "fc0").update({"in": 32})),
    ("fin>100", lambda c: (_w(c, "fc0").update({"in": 101, "out": 128}), _w(c, "efc0").update({"in": 128}),
                           _w(c, "efc1").update({"in": 128}))),
    ("heads>8", lambda c: [_w(c, k).update(heads=16) for k in ("efc0", "efc1")] + [
        _w(c, "fc0").update(out=64), _w(c, "efc0").update({"in": 64}), _w(c, "efc1").update({"in": 64})]),
    ("D=2", lambda c: (_w(c, "fc0").update({"in": 6, "out": 8}), _w(c, "efc0").update({"in": 8}),
                       _w(c, "efc1").update({"in": 8}))),
    ("hoisted", lambda c: c["nodes"][1].update(hoisted=True)),
    ("third reader", lambda c: c["nodes"].append(dict(c["nodes"][4], **{"in": [1], "out": 99}))),
    ("given source logit", lambda c: c["nodes"][3].update({"in": [2, 2, 1]})),
])
def test_predicate_refuses(ir, name, fn):
    assert _eligible(_edit(ir, fn)) == [False, False], name


def test_predicate_refuses_layout_partition_symmetry_and_switch(ir):
    class Chunked(_Part):
        chunks = 2
    assert _eligible(ir, layout_mode="vcut") == [False, False]
    assert _eligible(ir, part=object()) == [False, False]          # no own_offset (the vertex cut's)
    assert _eligible(ir, part=Chunked()) == [False, False]
    asked = []
    assert _eligible(ir, symmetric=lambda: asked.append(1) or False) == [False, False] and asked == [1]
    with _env(GALA_GAT_INPUT="0"):
        assert _eligible(ir, symmetric=lambda: asked.append(1) or True) == [False, False]
    assert asked == [1]                                            # refused before the transpose


@pytest.mark.parametrize("case,kw", [
    ("fin=H*D", dict(edit=("feature_size(20)", "feature_size(32)"))),
    ("vcut", dict(extra=("--layout", "vcut"))),
])
def test_ineligible_programs_run_on_the_stats_pair(runs, case, kw):
    """A run the predicate refuses reports "stats" for every layer and is the same run as with
    GALA_GAT_INPUT=0 (the parent's code path), exactly."""
    d, s = runs(1, iters=2, **kw)
    assert [k for _, k in kinds(s)] == ["stats", "stats"]
    d0, s0 = runs(1, switch="0", iters=2, **kw)
    np.testing.assert_array_equal(d["losses"], d0["losses"])
    np.testing.assert_array_equal(d["prediction"], d0["prediction"])
    assert s["gat_layers"] == s0["gat_layers"]


@pytest.mark.parametrize("prog,msg", [("gat_directed.txt", "directed GAT programs"),
                                      ("gat_fixed.txt", "FIXED-mode GAT")])
def test_refused_programs_stay_refused(runs, prog, msg):
    """check_program's refusals are untouched: directed and FIXED GAT programs (no input-space
    layer either) still end with NotImplementedError."""
    from gala import dist_run
    c = ref.load_ir(str(runs.ir(prog)))["post"]
    assert not any(_eligible(c))
    with pytest.raises(NotImplementedError, match=msg):
        dist_run.check_program(c, "halo")
    with pytest.raises(NotImplementedError, match="kernel-sampled GAT"):
        dist_run.check_program(_edit(ref.load_ir(str(runs.ir()))["post"], lambda c: c["sched"].update(kernel_sample=5)))
    with pytest.raises(AssertionError, match=msg):
        runs(1, iters=1, prog=prog)


# ---- the op itself ------------------------------------------------------------------------------
class _RecordingLayer:
    """Stands in for HaloGatInput in _GatInputLayer: backward must get a 16-byte aligned dY."""
    H = HEADS

    def __init__(self, n, fin, F):
        self.n, self.fin, self.F, self.seen = n, fin, F, []

    def forward_train(self, X, W, b, wL, bL, wR, bR, relu=False):
        return torch.zeros(self.n + 1, self.F)[1:].clone()

    def backward(self, dY):
        self.seen.append((dY.data_ptr() % 16, dY.is_contiguous(), dY.clone()))
        if dY.data_ptr() % 16:
            raise ValueError("gala_gat_in_bwd_rect_f32: dY is not 16-byte aligned")
        D = self.F // self.H
        return (torch.zeros(self.n, self.H), torch.ones(self.H, D, self.fin + 1),
                (torch.ones(self.H, self.fin), torch.ones(self.H)))


def test_unaligned_dy_is_cloned_before_the_backward():
    """A contiguous dY view at a 4-byte storage offset reaches the layer's backward as an aligned
    copy with the same values; the six gradients come back in the parameters' shapes, the two
    attention Linears' in separate storage."""
    from gala.dist_run import _GatInputLayer
    n, fin, F = 5, 20, 32
    layer = _RecordingLayer(n, fin, F)
    P = [torch.randn(s, requires_grad=True) for s in ((F, fin), (F,), (1, F), (HEADS,), (1, F), (HEADS,))]
    Y = _GatInputLayer.apply(*P, layer, True)
    base = torch.arange(n * F + 1, dtype=torch.float32)
    dY = base[1:].view(n, F)
    assert dY.is_contiguous() and dY.data_ptr() % 16 == 4
    Y.backward(dY)
    off, contig, seen = layer.seen[0]
    assert off == 0 and contig and torch.equal(seen, dY)
    for p in P:
        assert p.grad is not None and p.grad.shape == p.shape
    assert torch.equal(P[2].grad, P[4].grad) and P[2].grad.data_ptr() != P[4].grad.data_ptr()
    assert torch.equal(P[3].grad, P[5].grad) and P[3].grad.data_ptr() != P[5].grad.data_ptr()
