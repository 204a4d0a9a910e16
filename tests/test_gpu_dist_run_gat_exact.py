"""GPU: a FIXED GAT program under gala.dist_run on the HIP kernels (gala.dist.HaloGatExact over
gala_gat_fwd_stats_exact_ex_f32, gala_gat_bwd_exact_pre_ex_f32, gala_gat_bwd_exact_gather_ex_f32).

tests/dsl/gat_exact.txt (tests/test_dist_run_gat_exact_cpu.py) under GALA_DIST_GAT_EXACT=1 at
world 1 and on two ranks sharing the GPU over gloo, launched as tests/test_gpu_dist_run_gat_input.py
launches them (every rank a fresh child process under its own time limit; at most two processes
hold the GPU): both layers report "exact", two ranks equal one rank on the layer rows bit for bit,
and world 1 agrees with the host backend's run within the tolerance that file applies between the
backends (1e-4 on the layer rows, LOSS_TOL on the losses) and with the float64 IR semantics."""
import numpy as np
import pytest

from test_dist_run_cpu import _run
from test_dist_run_gat_exact_cpu import ITERS, PROG, SWITCH
from test_dist_run_gat_input_cpu import LOSS_TOL, PRED_TOL, Runs
from test_gpu_dist_run_gat_input import _run_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("gat_exact_gpu"), run=_run_gpu)


@pytest.fixture(scope="module")
def host_runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("gat_exact_host"), run=_run)


def _go(r, world):
    return r(world, iters=ITERS, prog=PROG, env=SWITCH)


def _keys(s):
    assert [e["kind"] for e in s["gat_layers"]] == ["exact", "exact"]
    return [f"gat_out:{e['node']}" for e in s["gat_layers"]]


def test_gpu_one_rank_exact_layers(runs, host_runs):
    d, s = _go(runs, 1)
    keys = _keys(s)
    assert s["loss_last"] < s["loss_first"] and all(e["halo_bytes_per_step"] == 0 for e in s["gat_layers"])
    dh, sh = _go(host_runs, 1)
    assert _keys(sh) == keys
    for k in keys:
        np.testing.assert_allclose(d[k], dh[k], rtol=1e-4, atol=1e-4, err_msg=k)
    np.testing.assert_allclose(d["losses"], dh["losses"], **LOSS_TOL)
    from _dist_check import check_dist_dump
    check_dist_dump(runs.ir(PROG), d)


def test_gpu_two_ranks_match_one(runs):
    a, s = _go(runs, 2)
    b, _ = _go(runs, 1)
    for k in _keys(s) + ["prediction"]:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert all(e["halo_bytes_per_step"] > 0 for e in s["gat_layers"])
    np.testing.assert_allclose(a["losses"], b["losses"], **LOSS_TOL)
    steps = [k for k in a if k.startswith("step1:")]
    assert steps
    for k in steps:
        np.testing.assert_allclose(a[k], b[k], err_msg=k, **PRED_TOL)
