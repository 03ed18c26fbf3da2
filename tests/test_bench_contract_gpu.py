"""GPU: bench.py's one-line JSON contract (the driver parses it), on a reduced workload so that the test takes seconds: the keys the
driver and the judge read, the lean plain line and its --dump-outputs files, the roofline and device objects of --full, the packed
variant."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, T=1024, steps=2):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--model", "0.1b", "--batch", "2", "--seq-len", str(T), "--steps", str(steps), "--warmup", "1",
           "--no-decode", "--no-cpu-baseline", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-500:]          # exactly ONE JSON line on stdout
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_bench_line_has_the_contract_keys():
    d = _run("--full")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "device", "kernel_ms"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "bf16" and d["data"] == "synthetic" and d["unit"] == "tokens/s"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 2 * 1024 * 2 / (d["ms_per_step"] * 2 * 1e-3)) < 1e-2 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r and "fwd_bwd" in r and "pmc_stale" in r
    assert r["algorithmic_bytes_per_launch"] == 13 * 64 * 2 * 2 * 1024 * 12      # 13 streams x 64 channels x bf16, B T H = 2 x 1024 x 12
    dev = d["device"]
    assert dev["compute_units"] == 256 and dev["wkv7_group_probe_ms"] > 0 and dev["step_over_wkv7_probe"] > 0


@pytest.mark.timeout(900)
def test_plain_bench_line_is_lean_and_dumps_the_last_timed_step(tmp_path):
    """Without --full the line holds the headline alone: --steps timed steps, no secondary measurement.  --dump-outputs writes the
    loss of the last timed step and samples of its gradients and weights as float32 .npy files, within 64 MB, and a second run
    with the same arguments writes the same bits."""
    import numpy as np
    d = _run("--dump-outputs", str(tmp_path / "out"), steps=3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "loss", "config"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert abs(d["value"] - 2 * 1024 * 3 / (d["ms_per_step"] * 3 * 1e-3)) < 1e-2 * d["value"]
    for k in ("roofline", "kernel_ms", "packed", "decode", "cpu_baseline", "comm"):
        assert k not in d, k
    assert "copy_probe_gbs" not in d["device"] and "wkv7_group_probe_ms" not in d["device"]
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["grad_sample.npy", "loss.npy", "master_sample.npy", "param_sample.npy"], files
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["loss"].shape == (1,) and abs(float(got["loss"][0]) - d["loss"]) < 1e-3
    n = len(got["grad_sample"])
    assert n > 0 and len(got["param_sample"]) == n and len(got["master_sample"]) == n and np.abs(got["grad_sample"]).max() > 0
    # the same arguments give the same inputs (batches and dropout masks), hence the same outputs, bit for bit
    again = _run("--dump-outputs", str(tmp_path / "again"), steps=3)
    assert again["loss"] == d["loss"]
    for f in files:
        assert np.array_equal(np.load(tmp_path / "again" / f), got[f[:-4]]), f


@pytest.mark.timeout(900)
def test_bench_packed_line_counts_real_tokens():
    d = _run("--packed", T=4096)
    lens = d["config"]["packed_lengths"]
    assert "PACKED" in d["config"]["workload"] and sum(lens) == 2 * 4096 - 32 * len(lens)
    assert abs(d["value"] - sum(lens) * 2 / (d["ms_per_step"] * 2 * 1e-3)) < 1e-2 * d["value"]


@pytest.mark.timeout(900)
def test_bench_default_line_carries_the_packed_object():
    """The --full N = 1 line measures the packed row too (after the timed region, outside `value`); --no-packed drops it."""
    d = _run("--full", T=4096)
    p = d["packed"]
    assert "error" not in p, p
    assert p["aligned_positions"] == 2 * 4096 and p["tokens"] == 2 * 4096 - 32 * p["sequences"] and p["unit"] == "tokens/s"
    assert abs(p["value"] - p["tokens"] / (p["ms_per_step"] * 1e-3)) < 1e-2 * p["value"]
    assert abs(d["value"] - 2 * 4096 * 2 / (d["ms_per_step"] * 2 * 1e-3)) < 1e-2 * d["value"]     # the headline is untouched by it
    assert "packed" not in _run("--full", "--no-packed", T=4096)


@pytest.mark.timeout(900)
def test_bench_two_ranks_in_the_drivers_launch_form():
    """REHEARSAL of the N > 1 path on a one-GPU box: the driver's own command line (torch.distributed.run ... bench.py --gpus 2), two
    ranks sharing GPU 0 over gloo (--one-device): process-group creation under its watchdog, preflight, steps, ONE JSON line from rank 0
    with `comm.preflight`.  Not a measurement."""
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--one-device", "--model", "0.1b", "--batch", "2", "--seq-len", "1024", "--steps", "2",
           "--warmup", "1", "--no-decode", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=800, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "packed" not in d and "decode" not in d
    assert abs(d["value"] - 2 * 2 * 1024 * 2 / (d["ms_per_step"] * 2 * 1e-3)) < 1e-2 * d["value"]      # whole-job tokens of both ranks
    pf = d["comm"]["preflight"]
    assert len(pf["ranks"]) == 2 and pf["allreduce_64mib"]["ms"] > 0 and "exposed_wait_ms_per_step" in d["comm"]
