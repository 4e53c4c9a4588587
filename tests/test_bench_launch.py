"""bench.py's own launcher (CPU): `python bench.py --gpus N` with no WORLD_SIZE must start its N ranks itself, as a child process,
and relay their outcome - not exit with a usage error, which is what the driver's N > 1 command line would have met."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_starts_its_own_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
                          "--no-extras"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    # no GPU in this container: both ranks were started (torch.distributed.run) and each says what it needs; the parent relays rc != 0
    assert out.returncode != 0
    assert "needs `python -m torch.distributed.run" not in text
    assert "bench.py needs an MI355X" in text or "this node shows" in text, text[-2000:]
    assert "torch.distributed" in text or "local_rank" in text, text[-2000:]          # the elastic launcher ran


def test_bench_quotes_counters_only_from_the_same_build():
    """profiles/<tag>_pmc.json records the library its counters were collected with (lib_sha16); bench.py's line quotes them only
    when the workload AND the library match - a kernel change without a fresh profile must not ship stale traffic / issue numbers."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    idx = json.load(open(os.path.join(ROOT, "profiles", "current.json")))
    prof = json.load(open(os.path.join(ROOT, "profiles", idx["pmc"])))
    assert prof.get("lib_sha16") and prof.get("workload")
    got = bench.load_profile(prof["workload"], prof["lib_sha16"])
    assert got is not None and got["_file"].endswith(idx["pmc"]) and got["kernels"]["k_tile<0>"]["hbm_bytes_per_frame"] > 0
    assert bench.load_profile(prof["workload"], "0" * 16) is None                      # another build of the library
    assert bench.load_profile(prof["workload"] + " [other]", prof["lib_sha16"]) is None  # another workload


def test_dump_outputs_writes_every_array_as_float32(tmp_path):
    """--dump-outputs DIR: the arrays of the last timed frame, whole, as DIR/<name>.npy in float32 (exact for 8-bit channels)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    arrays = {"color": rng.integers(0, 256, size=(30, 40, 4), dtype=np.uint8), "depth": rng.random((30, 40), dtype=np.float32),
              "shadowmap": rng.random((16, 16), dtype=np.float32)}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["color.npy", "depth.npy", "shadowmap.npy"]
    for k, v in arrays.items():
        got = np.load(str(tmp_path / (k + ".npy")))
        assert got.dtype == np.float32 and got.shape == v.shape and np.array_equal(got, v)


def test_dump_outputs_samples_the_same_pixels_under_the_size_limit(tmp_path):
    """Outputs larger than the limit: a fixed, seeded sample of each array's pixels plus their flat indices, within the limit, the
    same files from run to run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(2)
    arrays = {"color": rng.integers(0, 256, size=(60, 80, 4), dtype=np.uint8), "depth": rng.random((60, 80), dtype=np.float32)}
    limit = 40000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, limit=limit)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["color.npy", "color_index.npy", "depth.npy", "depth_index.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in names) <= limit
    for n in names:
        assert open(str(tmp_path / "a" / n), "rb").read() == open(str(tmp_path / "b" / n), "rb").read()
    for k, v in arrays.items():
        vals, idx = np.load(str(tmp_path / "a" / (k + ".npy"))), np.load(str(tmp_path / "a" / (k + "_index.npy")))
        assert vals.dtype == np.float32 and idx.dtype == np.float64 and len(vals) == len(idx) > 100
        assert np.all(np.diff(idx) > 0) and np.array_equal(vals, v.reshape(len(v) * v.shape[1], -1)[idx.astype(np.int64)])


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_from_run_to_run(tmp_path):
    """Two runs with the same arguments: the result line holds the steps asked for and ms_per_step, and the dumped frame, depth and
    shadow map are identical (the inputs are seeded; the renderer is deterministic)."""
    import json
    import numpy as np
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--instances", "500",
                              "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path / run)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        text = out.stdout.decode(errors="replace")
        assert out.returncode == 0, text[-3000:]
        line = json.loads([x for x in text.splitlines() if x.startswith("{")][-1])
        assert line["steps"] == 7 and line["ms_per_step"] > 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["color.npy", "depth.npy", "shadowmap.npy"] == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        a, b = np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n))
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    color, depth = np.load(str(tmp_path / "a" / "color.npy")), np.load(str(tmp_path / "a" / "depth.npy"))
    assert color.shape == (1080, 1920, 4) and depth.shape == (1080, 1920)
    assert np.array_equal(color, np.round(color)) and color.min() >= 0 and color.max() <= 255
    assert (depth < 1.0).sum() > 1000                                   # scene geometry in the frame
