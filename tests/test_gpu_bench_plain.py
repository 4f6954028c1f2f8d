"""`python bench.py --gpus 1` without --full: the headline line alone, and with --dump-outputs the last timed step's outputs, which
must be what the CPU checker computes for the same syndromes."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path, oracle_built):
    from ldpc_amd.codes import regular_ldpc_code
    from ldpc_amd.noise_models import generate_bsc_batch
    from test_gpu_async_group import _bench
    B, p = 4096, 0.09
    got = _bench(["--gpus", "1", "--batch-per-gpu", str(B), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert got["metric"] == "syndromes_per_sec_batched_bp50_product_sum_ldpc36_n10k" and got["unit"] == "syndromes/s"
    assert got["higher_is_better"] is True and got["dtype"] == "f64" and got["steps"] == 3 and got["warmup"] == 1
    assert abs(got["value"] - B / (got["ms_per_step"] * 1e-3)) < 1e-6 * got["value"]
    assert not {"roofline", "cpu_baseline", "host_io", "secondary", "parity_failed"} & set(got)

    files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(tmp_path, "*.npy"))}
    assert set(files) == {"rows", "decoding", "log_prob_ratios", "iterations", "converge"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(tmp_path, "*.npy"))) <= 64 << 20
    rows = files["rows"].astype(np.int64)
    assert files["iterations"].shape == (B,) and files["decoding"].shape == (len(rows), 10000)
    assert abs(float(files["iterations"].mean()) - got["config"]["mean_iterations"]) < 1e-9

    h = regular_ldpc_code(10000, 3, 6, seed=1)
    pick = rows[:12]
    err = np.concatenate([generate_bsc_batch(10000, p, 7, int(r), 1) for r in pick])
    synd = np.asarray((h.astype(np.int32) @ err.T.astype(np.int32)).T % 2, dtype=np.uint8)
    dec, llr, it, cv = oracle_built.BpOracle(h, error_rate=p, max_iter=50).decode_batch(synd)
    assert np.array_equal(files["decoding"][:12], dec.astype(np.float32))
    assert np.array_equal(files["iterations"][pick], it.astype(np.float32))
    assert np.array_equal(files["converge"][pick], cv.astype(np.float32))
    assert oracle_built.llr_close(files["log_prob_ratios"][:12], llr, rtol=1e-5)
