"""A SAGE student with max aggregation on two and four node-range shards sharing the one GPU (tools/checks/multirank_one_gpu.py,
``max_aggregation_cases``) against the single-GPU step: the real max-piece and gather-backward kernels with a non-empty halo, in both
exchange orders, with a rank that owns no train row, and with the column-sliced form forced (which max never takes).  The comparison
bars are the tool's (tests/test_gpu_multirank.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["sage-max-supervised-natural-ov1", "sage-max-kd-natural-ov0", "sage-max-lpw-community-ov1", "sage-max-kd-notrain-tail-ov1",
         "sage-max-kd-sliced-natural-ov1"]


def _run(world, tmp_path_factory):
    out = str(tmp_path_factory.mktemp(f"sharded_max{world}") / "report.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "checks", "multirank_one_gpu.py"), "--world", str(world), "--out", out,
                        "--cases", ",".join(CASES)], capture_output=True, text=True, timeout=180)
    return p, (json.load(open(out)) if os.path.exists(out) else {})


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    return _run(2, tmp_path_factory)


@pytest.fixture(scope="module")
def world4(tmp_path_factory):
    return _run(4, tmp_path_factory)


def _check(run, name):
    """The fields of tests/test_gpu_multirank.py::_check."""
    p, report = run
    assert name in report, (p.returncode, p.stdout[-2500:], p.stderr[-2500:])
    e = report[name]
    assert e["collectives_consistent"], e["collectives_mismatch"]
    # max has no column-sliced form: also the case that forces "sliced" moves its rows through the halo exchange
    assert all(i["n_halo"] > 0 and i["comm"]["halo_all_to_all_bytes_sent"] > 0 for i in e["per_rank"]), "the halo must not be empty"
    assert all(i["comm"].get("sliced_exchanges", 0) == 0 for i in e["per_rank"])
    assert e["loss_err_in_bars"] <= 1.0, (e["losses"], e["ref_losses"])          # |d| <= 2e-4 |ref| + 1e-6 over 3 steps x 3 terms
    assert e["logit_err_in_bars"] <= 1.0, e["logit_err_in_bars"]                 # |d| <= 1e-4 |ref| + 1e-5 max|ref|, initial eval
    assert e["acc_abs_err"] <= 1.5 * e["acc_one_node"], (e["accs"], e["ref_accs"])
    if "notrain" in name:
        assert e["per_rank"][-1]["n_train_local"] == 0 and e["per_rank"][0]["n_train_local"] > 0
    assert e["ok"]


@pytest.mark.parametrize("name", CASES)
def test_max_aggregation_on_two_ranks_matches_the_single_gpu_path(world2, name):
    _check(world2, name)


@pytest.mark.parametrize("name", CASES)
def test_max_aggregation_on_four_ranks_matches_the_single_gpu_path(world4, name):
    _check(world4, name)


def test_max_aggregation_multirank_processes_ended_cleanly(world2, world4):
    for world, (p, report) in ((2, world2), (4, world4)):
        assert p.returncode == 0 and "MULTIRANK-OK" in p.stdout, (p.returncode, p.stdout[-2500:], p.stderr[-2500:])
        assert len(report) == len(CASES)
