"""CPU: bench.py's launch contract.  `--gpus N` must never quietly run fewer ranks than asked for: a mismatch with the
launcher's WORLD_SIZE is an error, and on a box that cannot host N ranks the self-launched run fails loudly (non-zero
exit, no JSON line) instead of printing an n_gpus=1 line.  GPU (marked): a plain run's line and its --dump-outputs."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_gpus_must_match_world_size():
    for gpus, world in (("2", "4"), ("8", "1"), ("1", "2")):
        r = subprocess.run([sys.executable, BENCH, "--gpus", gpus], env=_env(WORLD_SIZE=world), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "WORLD_SIZE" in r.stderr and r.stdout.strip() == ""


def test_self_launch_fails_loudly_without_enough_gpus():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this box could really host two ranks")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rows", "2048", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0, r.stdout
    assert "2-GPU run failed" in r.stderr
    assert "n_gpus" not in r.stdout  # no benchmark line from a run that did not happen


def test_parity_gate_rejects_a_wrong_result(oracle):
    """bench.parity_rescore — the gate in front of the timed region — accepts the oracle's own top-k of regenerated rows
    and ends the run (SystemExit, non-zero) when a score bit, the order or a row is wrong."""
    import numpy as np
    import pytest
    sys.path.insert(0, ROOT)
    import bench
    from otters_amd._native import HIT_DTYPE
    dim, seed, n, k = 48, 0x07735, 5000, 10
    rows = oracle.rand_rows(0, n, dim, seed)
    q = np.random.default_rng(3).uniform(-1, 1, dim).astype(np.float32)
    ref = oracle.vec_query(rows, q, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, ties=oracle.TIES_CANONICAL)
    hits = np.zeros(k, dtype=HIT_DTYPE)
    hits["index"], hits["score"], hits["query"] = ref["index"], ref["score"], 0
    bench.parity_rescore(hits, q, dim, seed)  # the truth passes
    bad = hits.copy()
    bad["score"][3] = np.nextafter(bad["score"][3], np.float32(2.0))  # one ulp off
    with pytest.raises(SystemExit) as e:
        bench.parity_rescore(bad, q, dim, seed)
    assert "PARITY FAILED" in str(e.value)
    bad = hits.copy()
    bad[[2, 3]] = bad[[3, 2]]  # right rows and scores, wrong order
    with pytest.raises(SystemExit):
        bench.parity_rescore(bad, q, dim, seed)
    bad = hits.copy()
    bad["index"][0] = bad["index"][1]  # a row twice
    with pytest.raises(SystemExit):
        bench.parity_rescore(bad, q, dim, seed)
    bad = hits.copy()
    bad["index"][5] = (int(bad["index"][5]) + 1) % n  # a different row under the same score
    with pytest.raises(SystemExit):
        bench.parity_rescore(bad, q, dim, seed)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(oracle, tmp_path):
    """A plain run (no --full) prints the headline line with `ms_per_step` over exactly --steps timed steps and none of what
    --full adds; --dump-outputs writes the last timed step's hits, which are the oracle's top-k of that step's query over the
    regenerated rows, index for index and bit for bit."""
    import json
    import numpy as np
    rows, dim, k, seed, steps, warmup = 20480, 96, 10, 0x07735, 3, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--rows", str(rows), "--dim", str(dim), "--k", str(k), "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)], env=_env(), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0 and d["n_gpus"] == 1, d
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f32", d
    assert abs(d["value"] - rows * (dim * 4 + 4) / (d["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * d["value"], d
    assert d["parity_checked"] is False and "extras" not in d and "cpu_baseline" not in d and d["roofline"]["traffic"] is None, d
    got = {name: np.load(out / f"{name}.npy") for name in ("index", "score", "query")}
    assert got["index"].dtype == np.float64 and got["score"].dtype == np.float32 and got["query"].dtype == np.float64
    q = np.random.default_rng(seed + 1).uniform(-1, 1, (steps + warmup, dim)).astype(np.float32)[-1]
    ref = oracle.vec_query(oracle.rand_rows(0, rows, dim, seed), q, oracle.METRIC_COSINE, oracle.TAKE_MAX, k, ties=oracle.TIES_CANONICAL)
    assert np.array_equal(got["index"], ref["index"].astype(np.float64)), (got["index"], ref["index"])
    assert np.array_equal(got["score"].view(np.uint32), np.asarray(ref["score"], np.float32).view(np.uint32))
    assert np.array_equal(got["query"], np.zeros(k))
