"""bench.py's plain run and `--dump-outputs`.

A plain run times its steps and prints the headline line only; what else the benchmark measures sits behind `--full`.
`--dump-outputs DIR` writes what the last timed step computed — the gathered image and the step's ray count — so that
two builds can be compared output for output: the files must be float32 / float64, at most 64 MB together (a larger
image is cut to a fixed, seeded row sample), and the same from run to run.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench

ROOT = Path(__file__).resolve().parents[1]


def test_dump_outputs_whole_image_and_seeded_row_sample(tmp_path, monkeypatch):
    import torch

    img = torch.arange(37 * 5 * 3, dtype=torch.float32).reshape(37, 5, 3)
    shapes = bench.dump_outputs(str(tmp_path / "whole"), img, 12345)
    assert shapes == {"rays": [1], "image": [37, 5, 3]}
    got = np.load(tmp_path / "whole" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img.numpy())
    rays = np.load(tmp_path / "whole" / "rays.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [12345.0]
    assert sorted(f.name for f in (tmp_path / "whole").iterdir()) == ["image.npy", "rays.npy"]

    # above the limit: whole rows, a fixed seeded choice in ascending order, named by image_rows; all within the limit
    limit = 1000
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img, 7)
    a = {f.stem: np.load(f) for f in (tmp_path / "a").iterdir()}
    b = {f.stem: np.load(f) for f in (tmp_path / "b").iterdir()}
    assert set(a) == {"image", "image_rows", "rays"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= limit
    rows = a["image_rows"].astype(np.int64)
    assert 0 < len(rows) < 37 and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 37
    # (as many rows as fit: one more row would pass the limit)
    assert sum(v.nbytes for v in a.values()) + img[0].numpy().nbytes > limit
    assert np.array_equal(a["image"], img.numpy()[rows])
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path):
    """One plain run of a small C3 crop: --steps sets the number of timed steps, the line carries the headline fields and
    none of the `--full` blocks, and the dumped image and ray count equal a renderer drawing the same step here."""
    import hrt
    import scenes

    if hrt.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box (there is no CPU fallback)")
    W, H, F = 72, 40, 3
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--width", str(W), "--height", str(H), "--frames", str(F), "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert (res["steps"], res["warmup"], res["unit"], res["higher_is_better"], res["dtype"]) == (2, 1, "Mrays/s", True, "f32")
    assert res["ms_per_step"] > 0 and res["value"] > 0 and "Mrays/sec" in res["metric"]
    assert " step 1:" in out.stderr and " step 2:" not in out.stderr  # (the log names every timed step)
    for moved in ("cpu_baseline", "golden", "emulated_split", "c5"):
        assert moved not in res

    sd = scenes.CONFIGS["c3"]()
    sd.width, sd.height, sd.frames = W, H, F
    r = scenes.make_renderer(sd)
    r.set_params(**bench.timed_knobs())
    r.draw_frames(sd.frames, bench.TIME0, bench.DTIME)
    img = np.load(tmp_path / "image.npy")
    assert img.dtype == np.float32 and img.shape == (H, W, 3)
    assert np.array_equal(img.view(np.uint32), r.read_image().view(np.uint32))
    assert np.load(tmp_path / "rays.npy").tolist() == [float(r.stats().queries)] == [float(res["config"]["rays_per_step"])]
