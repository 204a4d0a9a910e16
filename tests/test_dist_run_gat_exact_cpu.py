"""CPU (host backend, gloo): a FIXED GAT program under gala.dist_run.

tests/dsl/gat_exact.txt (two layers, 8 heads in layer 1, gat_fixed_gradients(true)) on the
undirected synthetic graph: both GAT layers run through gala.dist.HaloGatExact (the exact pair over
the row partition), the summary's gat_layers says "exact", the layer rows of 2 and 3 ranks are
bit-identical to one rank's, and one rank matches the float64 semantics of the IR -- the TRUE
gradients of the stable softmax -- at the tolerance the other dist_run GAT tests use
(tests/_dist_check.py).  What is still refused has one negative case each: the vertex cut, a
directed program, kernel sampling, a graph whose pattern is not symmetric.

FIXED programs run under GALA_DIST_GAT_EXACT=1; without the switch check_program refuses them as
it did before HaloGatExact (tests/test_dist_run_gat_input_cpu.py keeps asserting that), which is
also what it did with the switch then: this file cannot pass on the code before HaloGatExact."""
import json
import os

import numpy as np
import pytest

import _graphs as G
import _ir_ref as ref
from _dist_check import check_dist_dump
from test_dist_run_gat_input_cpu import LOSS_TOL, PRED_TOL, Runs, _env

PROG = "gat_exact.txt"
ITERS = 3


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("gat_exact"))


SWITCH = {"GALA_DIST_GAT_EXACT": "1"}


def _run(runs, world):
    return runs(world, iters=ITERS, prog=PROG, env=SWITCH)


@pytest.fixture
def switch_on():
    old = os.environ.get("GALA_DIST_GAT_EXACT")
    os.environ["GALA_DIST_GAT_EXACT"] = "1"
    yield
    os.environ.pop("GALA_DIST_GAT_EXACT", None)
    if old is not None:
        os.environ["GALA_DIST_GAT_EXACT"] = old


@pytest.mark.parametrize("world", [1, 2, 3])
def test_run_takes_the_exact_layers(runs, world):
    d, s = _run(runs, world)
    assert [e["kind"] for e in s["gat_layers"]] == ["exact", "exact"]
    assert all(not e["tmode"] and e["setup_bytes"] == 0 for e in s["gat_layers"])
    assert s["loss_last"] < s["loss_first"]
    if world == 1:
        assert all(e["halo_bytes_per_step"] == 0 for e in s["gat_layers"])
        return
    from gala import dist as gdist
    from gala import layout
    g = layout.HostGraph(len(d["rowptr"]) - 1, len(d["rowptr"]) - 1, d["rowptr"], d["col"])
    part = gdist.partition_graph(g, 0, world)
    e1, e2 = s["gat_layers"]        # layer 1: F = 8 * 32, H = 8; layer 2: F = 7, H = 1 (derived, not measured)
    assert e1["halo_bytes_per_step"] == part.halo_bytes(2 * 256 + 8 + 4 * 8) > 0
    assert e2["halo_bytes_per_step"] == part.halo_bytes(2 * 7 + 1 + 4 * 1)


def test_one_rank_matches_ir_semantics(runs):
    """World 1 against the float64 executor of the IR (FIXED: the stable softmax and autograd's
    true gradients): predictions, loss and the first epoch's weight gradients."""
    d, _ = _run(runs, 1)
    ir = ref.load_ir(str(runs.ir(PROG)))["post"]
    assert ir["sched"]["gat_mode"] != 0 and ir["sched"]["undirected"]
    check_dist_dump(runs.ir(PROG), d)


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_match_one_rank_bit_for_bit(runs, world):
    """The GAT layers' rows and the predictions of N ranks equal one rank's bit for bit; the loss
    curve and the parameters after one step within the cross-rank sums' rounding."""
    a, s = _run(runs, world)
    b, _ = _run(runs, 1)
    keys = [f"gat_out:{e['node']}" for e in s["gat_layers"]]
    assert len(keys) == 2
    for k in keys + ["prediction"]:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_allclose(a["losses"], b["losses"], **LOSS_TOL)
    steps = [k for k in a if k.startswith("step1:")]
    assert steps and sorted(steps) == sorted(k for k in b if k.startswith("step1:"))
    for k in steps:
        np.testing.assert_allclose(a[k], b[k], err_msg=k, **PRED_TOL)


def _edit(ir, **sched):
    c = json.loads(json.dumps(ir))
    c["sched"].update(sched)
    return c


def test_off_without_the_switch(runs):
    from gala import dist_run
    ir = ref.load_ir(str(runs.ir(PROG)))["post"]
    with _env(GALA_DIST_GAT_EXACT=None):      # unset, whatever the caller's environment holds
        assert not dist_run.gat_exact_enabled()
        with pytest.raises(NotImplementedError, match="GALA_DIST_GAT_EXACT=1"):
            dist_run.check_program(ir, "halo")


def test_what_is_still_refused(runs, switch_on):
    from gala import dist_run
    ir = ref.load_ir(str(runs.ir(PROG)))["post"]
    dist_run.check_program(ir, "halo")
    with pytest.raises(NotImplementedError, match="the cut splits rows"):
        dist_run.check_program(ir, "vcut")
    directed = _edit(ref.load_ir(str(runs.ir("gat_directed.txt")))["post"], gat_mode=1)
    assert not directed["sched"]["undirected"]
    with pytest.raises(NotImplementedError, match="directed FIXED-mode GAT"):
        dist_run.check_program(directed, "halo")
    with pytest.raises(NotImplementedError, match="kernel-sampled FIXED-mode GAT"):
        dist_run.check_program(_edit(ir, kernel_sample=5), "halo")
    # the input-space layer stays REF-only
    plan = dist_run.plan_input_layers(ir)
    assert not any(dist_run.input_layer_eligible(ir, n, plan, "halo", None, True)
                   for n in ir["nodes"] if n["op"] == "GAT_AGGREGATE")
    # a graph whose pattern is not symmetric: refused when the program is built, before any layer
    g = G.with_empty_rows()
    assert not dist_run.pattern_is_symmetric(g)
    with pytest.raises(NotImplementedError, match="not symmetric"):
        dist_run.Program(ir, g, None, None, None, 0, 1, "cpu")
