"""bench.py as the driver runs it (``--gpus 1 --steps K --warmup W``), rehearsed on CPU with the tiny model: the result
line's headline fields, ``--steps`` setting the number of timed steps, and ``--dump-outputs`` / ``--full``."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("loss", "grad_norm", "params_sample", "exp_avg_sample")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                              "MASTER_PORT")}
    env.update(DLLM_FORCE_CPU="1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "t5-tiny", "--warmup", "1",
           "--batch-per-gpu", "2", "--src-len", "32", "--tgt-len", "8", *extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in DUMPED)
    return {n: np.load(os.path.join(d, n + ".npy")) for n in DUMPED}


def test_bench_dump_outputs_repeatable(tmp_path):
    """Two runs with the same arguments (one of them with ``--full``, which a 1-GPU run has nothing to add to) write
    the same float32 arrays: inputs, initial weights and dropout are seeded.  One more timed step changes them: the dump
    is the LAST timed step's, and ``--steps`` sets how many there are."""
    a, b, c = (str(tmp_path / n) for n in "abc")
    da = _bench("--steps", "2", "--dump-outputs", a)
    db = _bench("--steps", "2", "--full", "--dump-outputs", b)
    dc = _bench("--steps", "3", "--dump-outputs", c)
    for d, steps in ((da, 2), (db, 2), (dc, 3)):
        assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
        assert d["ms_per_step"] > 0
        # the headline is the timed steps' throughput: batch 2 per step of ms_per_step milliseconds
        assert abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    xa, xb, xc = _load(a), _load(b), _load(c)
    for n in DUMPED:
        assert xa[n].dtype == np.float32 and np.isfinite(xa[n]).all()
        np.testing.assert_array_equal(xa[n], xb[n])
    assert xa["loss"].shape == (1,) and xa["grad_norm"].shape == (1,) and xa["grad_norm"][0] > 0
    assert xa["params_sample"].shape == xa["exp_avg_sample"].shape and xa["params_sample"].size > 1000
    assert np.abs(xa["exp_avg_sample"]).max() > 0  # the optimizer state of a step that ran
    assert sum(x.nbytes for x in xa.values()) <= 64 * 2**20
    assert not np.array_equal(xa["params_sample"], xc["params_sample"])
    assert xa["loss"][0] != xc["loss"][0]


def test_bench_dump_sample_is_fixed_and_bounded():
    """Past DUMP_SAMPLE elements the dump is a sample at offsets drawn from the seed alone: sorted, in range, the same
    on every call, so two builds are compared at the same weights."""
    import torch

    import bench

    class _Opt:
        pass

    class _Eng:
        pass

    n = bench.DUMP_SAMPLE + 12345
    eng, opt = _Eng(), _Opt()
    opt.master = torch.arange(n, dtype=torch.float32)
    opt.exp_avg = -torch.arange(n, dtype=torch.float32)
    eng.optimizer = opt
    eng.flat = None
    import tempfile
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        bench.dump_outputs(d1, eng, torch.tensor(1.5), torch.tensor(2.5), seed=0)
        bench.dump_outputs(d2, eng, torch.tensor(1.5), None, seed=0)
        x1, p2 = _load(d1), np.load(os.path.join(d2, "params_sample.npy"))
        assert not os.path.exists(os.path.join(d2, "grad_norm.npy"))  # a step without clipping reports no norm
    idx = x1["params_sample"]
    assert idx.shape == (bench.DUMP_SAMPLE,) and (np.diff(idx) >= 0).all() and 0 <= idx[0] and idx[-1] < n
    np.testing.assert_array_equal(idx, p2)
    np.testing.assert_array_equal(x1["exp_avg_sample"], -idx)
    assert x1["loss"][0] == 1.5 and x1["grad_norm"][0] == 2.5
