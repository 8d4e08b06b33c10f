"""bench.py's plain run and --dump-outputs: the headline alone, and the frame of the last timed step as arrays that another build's
run can be compared with."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as ou

sys.path.insert(0, ou.ROOT)


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    import bench
    rgba = np.random.default_rng(1).integers(0, 256, size=(1024, 2304, 4), dtype=np.uint8)     # more pixels than the bound: a sample
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rgba)
    px, idx = np.load(tmp_path / "a" / "frame_rgba.npy"), np.load(tmp_path / "a" / "frame_pixel_index.npy")
    assert px.dtype == np.float32 and idx.dtype == np.float64 and px.shape == (bench.DUMP_MAX_PIXELS, 4)
    assert (np.diff(idx) > 0).all() and idx[-1] < 1024 * 2304
    assert np.array_equal(idx, np.load(tmp_path / "b" / "frame_pixel_index.npy"))             # the same sample on every run
    assert np.array_equal(px, rgba.reshape(-1, 4)[idx.astype(np.int64)].astype(np.float32))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
    small = rgba[:90, :160]                                                                    # a small frame: every pixel, in order
    bench.dump_outputs(str(tmp_path / "c"), small)
    assert np.array_equal(np.load(tmp_path / "c" / "frame_rgba.npy"), small.reshape(-1, 4).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "c" / "frame_pixel_index.npy"), np.arange(90 * 160, dtype=np.float64))


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_frame(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "RT_BENCH_REHEARSE")}
    r = subprocess.run([sys.executable, os.path.join(ou.ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 7 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["metric"] == "Mpixel/s" and out["unit"] == "Mpixel/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert abs(out["value"] - 3840 * 2160 / (out["ms_per_step"] * 1e3)) <= 0.01 * out["value"]
    assert not {"roofline", "parity_ok", "cold_frame", "reference_scene", "cpu_baseline"} & set(out)     # only with --full
    px = np.load(tmp_path / "frame_rgba.npy")
    idx = np.load(tmp_path / "frame_pixel_index.npy").astype(np.int64)
    assert px.dtype == np.float32 and len(px) == len(idx) and (px[:, 3] == 255).all()
    # the sampled pixels that lie on the rows the reference itself rendered
    f = next(f for f in ou.manifest()["frames"] if f["name"] == "h8_3840x2160_rows")
    gold = ou.golden_frame(f).reshape(len(f["rows"]), f["w"], 4).astype(np.float32)
    y, x = idx // f["w"], idx % f["w"]
    seen = 0
    for k, row in enumerate(f["rows"]):
        on = y == row
        seen += int(on.sum())
        assert np.abs(px[on] - gold[k, x[on]]).max(initial=0) <= 1, row
    assert seen > 1000
