"""The data-parallel MAG epoch (dist.mag_dp_train_epoch) on two and four ranks sharing the one GPU over ``hostcomm``
(tools/checks/mag_dp_one_gpu.py): the real summing row step on the gathered batch rows of all ranks, 6 batches (four ranks leave a
partial last round), modes supervised / kd / nce, dropout seeded per batch -- and the whole path once with one rank over RCCL.  Every
run is a fresh child process with its own time limit; after a run that did not end cleanly no further run is started."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["supervised", "kd", "nce"]
_FAILED = []          # a run that did not end cleanly: nothing further is started on the GPU


def _run(world, backend, tmp_path_factory):
    if _FAILED:
        pytest.fail(f"not started: an earlier run did not end cleanly ({_FAILED[0]})")
    out = str(tmp_path_factory.mktemp(f"mag_dp_{backend}{world}") / "report.json")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "checks", "mag_dp_one_gpu.py"), "--world", str(world), "--backend", backend, "--out", out]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=170)
    except subprocess.TimeoutExpired as e:
        _FAILED.append(f"world {world} over {backend}: time limit")
        pytest.fail(f"{_FAILED[0]}: {str(e.stdout)[-2000:]} {str(e.stderr)[-2000:]}")
    if p.returncode != 0:
        _FAILED.append(f"world {world} over {backend}: exit code {p.returncode}")
    return p, (json.load(open(out)) if os.path.exists(out) else {})


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    return _run(2, "gloo", tmp_path_factory)


@pytest.fixture(scope="module")
def world4(tmp_path_factory):
    return _run(4, "gloo", tmp_path_factory)


@pytest.fixture(scope="module")
def rccl1(tmp_path_factory):
    return _run(1, "nccl", tmp_path_factory)


def _check(run, mode, world):
    p, report = run
    assert mode in report, (p.returncode, p.stdout[-2500:], p.stderr[-2500:])
    e = report[mode]
    print(f"[mag dp w={world} {mode}] spread={e['spread']:.3e} worst err={e['worst_err']:.3e} bound={e['worst_bound']:.3e} "
          f"shared rows per round={e['shared_rows_per_round']} payload={e['payload_bytes']}")
    assert e["replicas_identical"] and e["losses_identical"], "dense parameters, tables, m, v, last: equal checksums on every rank"
    assert e["within_bound"], (e["worst_err"], e["worst_bound"], e["spread"])      # 4 x spread of the two dense-Adam runs + one ulp
    assert e["collectives_mismatch"] is None, e["collectives_mismatch"]
    assert max(e["shared_rows_per_round"]) > 0, "no table row was named by two ranks in one round"
    assert e["rows_gathered"] == e["rows_expected"]
    assert e["payload_bytes"] == e["payload_expected"]                              # sum(n_r) * (4 D + 16) per step
    assert e["gather_bytes_traced"] == e["gather_bytes_padded_expected"]
    assert e["partial_last_round"] == (world == 4)
    if world == 4:
        assert e["rows_gathered"][-1][2:] == [0, 0], "two ranks of the last round have no batch and still step"
    assert e["ok"]


@pytest.mark.parametrize("mode", MODES)
def test_two_ranks_stay_identical_and_match_the_accumulated_epoch(world2, mode):
    _check(world2, mode, 2)


@pytest.mark.parametrize("mode", MODES)
def test_four_ranks_with_a_partial_last_round(world4, mode):
    _check(world4, mode, 4)


@pytest.mark.parametrize("mode", MODES)
def test_one_rank_over_rccl_equals_the_single_process_epoch_bitwise(rccl1, mode):
    p, report = rccl1
    assert mode in report, (p.returncode, p.stdout[-2500:], p.stderr[-2500:])
    e = report[mode]
    assert e["backend"] == "nccl" and e["gathers_traced"] == 3 * len(e["rounds"]) == 18
    assert e["equals_single_process_bitwise"] and e["losses"] == pytest.approx(e["ref_losses"], rel=1e-6)
    assert e["collectives_mismatch"] is None and e["payload_bytes"] == e["payload_expected"]
    assert e["ok"]


def test_processes_ended_cleanly(world2, world4, rccl1):
    for name, (p, report) in (("w2", world2), ("w4", world4), ("rccl1", rccl1)):
        assert p.returncode == 0 and "MAG-DP-OK" in p.stdout, (name, p.returncode, p.stdout[-2500:], p.stderr[-2500:])
        assert len(report) == len(MODES)
