"""bench.py's command line: --dump-outputs writes the arrays the last timed step returned (float64, a
fixed seeded sample of the large ones), and a plain run -- no --full -- prints the headline line alone.
The GPU case runs the benchmark once at a small odd shape and compares the dumped arrays with the
oracle's route + stable bucketing of the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BALANCED_GENS = [138558, 165678, 215136, 61804, 17808, 48728, 207265, 76820]   # bench.py SILO_SETS["balanced"]


def test_dump_outputs_float64_fixed_sample(tmp_path):
    import bench
    n = 3 * bench.DUMP_SAMPLE + 7
    big = (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 32)).astype(np.uint32)
    arrays = {"big": big.view(np.int32), "small": (np.arange(1000) % 251).astype(np.uint8), "absent": None,
              "empty": np.empty(0, np.uint32)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    assert sorted(os.listdir(a)) == ["big.npy", "empty.npy", "small.npy"]
    got = {f[:-4]: np.load(a / f) for f in os.listdir(a)}
    assert all(v.dtype == np.float64 for v in got.values())
    np.testing.assert_array_equal(got["small"], np.arange(1000) % 251)
    assert got["empty"].shape == (0,)
    # the sample: DUMP_SAMPLE elements of the array, in position order, uint32 values (not int32's
    # negatives), the same positions on every call
    assert got["big"].shape == (bench.DUMP_SAMPLE,) and got["big"].min() >= 0
    idx = np.sort(np.random.default_rng(0x5EED0D00 + n).integers(0, n, size=bench.DUMP_SAMPLE, dtype=np.int64))
    np.testing.assert_array_equal(got["big"], big[idx].astype(np.float64))
    np.testing.assert_array_equal(np.load(b / "big.npy"), got["big"])
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 << 20


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gpu_available, tmp_path):
    G, N, steps = 5003, 200001, 3
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--grains", str(G), "--msgs", str(N), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["metric"] == "routed messages/sec (lookup+bucket, whole node)" and line["unit"] == "messages/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32/u64 integer"
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-3)
    # the plain run measures nothing beside the headline, and leaves no record behind
    assert line["roofline"] is None and line["cpu_baseline"] is None and "secondary" not in line
    assert "full_record" not in line
    assert line["routed_ok_last_step_rank0"] == N

    silos = [o.Silo(f"10.0.0.{i + 1}", 11111, gen) for i, gen in enumerate(BALANCED_GENS)]
    spec = o.ring_spec(silos, "D")
    tc = o.grain_type_code(o.PING_GRAIN_CLASS)
    reg = o.grain_keys(tc, np.arange(G))
    owner = o.ring_owner_np(spec, o.jenkins_u64x3_np(reg[:, 2], reg[:, 0], reg[:, 1])).astype(np.uint32)
    ks = np.random.default_rng(0x5EED0001).integers(0, G, size=N, dtype=np.int64)
    want = o.route_batch_np(o.grain_keys(tc, ks), spec, o.DirectoryArrays(reg, np.arange(G), owner))
    wp, wo = o.bucket_stable(want[2], G)
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npy"))
    assert files == ["act.npy", "offsets.npy", "perm.npy", "silo.npy", "status.npy"]
    for name, w in (("status", want[0]), ("silo", want[1]), ("act", want[2]), ("perm", wp), ("offsets", wo)):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, np.asarray(w).astype(np.float64), err_msg=name)
