"""GPU: a GAT program's first layer in input space under gala.dist_run, on the HIP kernels
(gala_gat_in_*: T mode, and with GALA_GAT_IN_T=0 the walk).

tests/dsl/gat_input.txt (tests/test_dist_run_gat_input_cpu.py) at world 1 with T mode on and
off, and on two ranks sharing the GPU over gloo (RCCL needs one device per rank): the summary
names the input-space layer, it agrees with the three ops (GALA_GAT_INPUT=0) within the
tolerance tests/test_dist_run_cpu.py applies between layouts of a GAT program, with the host
backend's run of the same program within 1e-4 on the layer-1 rows, and two ranks are
bit-identical to one.  The same on an R-MAT graph with a row past the hub-row threshold.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_dist_run_cpu import PKG, ROOT, _free_port, _run
from test_dist_run_gat_input_cpu import HEADS, ITERS, L1, L2, LOSS_TOL, Runs, check_pair, kinds

pytestmark = pytest.mark.gpu

RANK_LIMIT_S = 200      # every rank's own time limit (timeout -k), below the launcher's


def _run_gpu(ir, tmp_path, world, tag, iters=ITERS, extra=()):
    """One gala.dist_run launch on the GPU: (dump, summary).  Two ranks share the device over
    gloo under torch.distributed.run, which ends every rank at the first failure; each rank
    runs under its own time limit."""
    dump = tmp_path / f"{tag}.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = PKG + os.pathsep + env.get("PYTHONPATH", "")
    env["GALA_DIST_BACKEND"] = "gloo"
    rank = ["timeout", "-k", "10", str(RANK_LIMIT_S), sys.executable, "-m", "gala.dist_run"]
    if world > 1:
        assert world == 2
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", "--no-python"] + rank
    else:
        cmd = rank
    cmd += [str(ir), "--synthetic", "--device", "cuda", "--iters", str(iters), "--dump", str(dump), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=RANK_LIMIT_S + 40, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert summary["ranks"] == world
    return dict(np.load(dump)), summary


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("gat_input_gpu"), run=_run_gpu)


@pytest.fixture(scope="module")
def host_runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("gat_input_host"), run=_run)


WALK = {"GALA_GAT_IN_T": "0"}


@pytest.mark.parametrize("tmode", [True, False])
def test_gpu_one_rank_input_space(runs, host_runs, tmode):
    """World 1 over the HIP backend, T mode on / off: the layer ran ("input", tmode as asked;
    layer 2 "stats"), agrees with the three ops of the same backend and with the host backend's
    input-space run (layer-1 rows within 1e-4)."""
    d, s = runs(1, env=None if tmode else WALK)
    assert kinds(s) == [(L1, "input"), (L2, "stats")]
    assert s["gat_layers"][0]["tmode"] is tmode and s["gat_layers"][1]["tmode"] is False
    assert s["gat_layers"][0]["halo_bytes_per_step"] == 0 and s["loss_last"] < s["loss_first"]
    d0, s0 = runs(1, switch="0")
    assert [k for _, k in kinds(s0)] == ["stats", "stats"]
    check_pair(d, d0)
    dh, sh = host_runs(1)
    assert kinds(sh) == kinds(s)
    np.testing.assert_allclose(d[f"gat_out:{L1}"], dh[f"gat_out:{L1}"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(d["losses"], dh["losses"], **LOSS_TOL)


def test_gpu_one_rank_matches_ir_semantics(runs):
    """T mode at world 1 against the float64 executor of the IR: forward, loss, gradients."""
    from _dist_check import check_dist_dump
    check_dist_dump(runs.ir(), runs(1)[0])


def test_gpu_two_ranks_match_one(runs):
    """Two ranks on the one GPU over gloo (T mode): q of the halo rows crosses once per
    training forward, the layer-1 rows and the predictions are bit-identical to one rank."""
    d, s = runs(2)
    assert kinds(s) == [(L1, "input"), (L2, "stats")] and s["gat_layers"][0]["tmode"] is True
    from gala import dist as gdist
    from gala import layout
    n = len(d["rowptr"]) - 1
    part = gdist.partition_graph(layout.HostGraph(n, n, d["rowptr"], d["col"]), 0, 2)
    assert s["gat_layers"][0]["halo_bytes_per_step"] == 4 * HEADS * part.n_halo_rows > 0
    assert s["q_exchanges"] == ITERS
    check_pair(d, runs(1)[0], bitwise_rows=True)


@pytest.mark.parametrize("world", [1, 2])
def test_gpu_rmat_hub_row_graph(runs, world):
    """The R-MAT graph with a hub row (the whole graph's chunks, on every rank): input space in
    T mode against the three ops, and two ranks bit-identical to one."""
    d, s = runs(world, extra=runs.rmat())
    assert kinds(s) == [(L1, "input"), (L2, "stats")] and s["gat_layers"][0]["tmode"] is True
    if world == 1:
        check_pair(d, runs(1, switch="0", extra=runs.rmat())[0])
        check_pair(d, runs(1, extra=runs.rmat(), env=WALK)[0])
    else:
        check_pair(d, runs(1, extra=runs.rmat())[0], bitwise_rows=True)
