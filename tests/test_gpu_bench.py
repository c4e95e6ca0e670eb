"""bench.py's command line on MI355X: the plain result line, --full, and
--dump-outputs (tiny batch, in-process so the suite pays no extra start-up).
"""

import json

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

CLIPS = 4


def run_bench(monkeypatch, capsys, *flags: str) -> dict:
    monkeypatch.setattr(
        "sys.argv",
        ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
         "--clips", str(CLIPS), *flags],
    )
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_prints_headline_only_and_dumps_outputs(monkeypatch, capsys, tmp_path):
    out = run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "dump"))
    assert out["unit"] == "clips/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["steps"] == 2
    assert out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert out["value"] == pytest.approx(CLIPS / (out["ms_per_step"] / 1e3), rel=1e-3)
    assert "roofline" not in out and "cpu_baseline" not in out

    files = sorted(p.name for p in (tmp_path / "dump").iterdir())
    assert files == ["clip_embeddings.npy"]
    emb = np.load(tmp_path / "dump" / "clip_embeddings.npy")
    assert emb.shape == (CLIPS, 512) and emb.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-5)

    # same arguments -> same inputs -> same outputs
    again = tmp_path / "again"
    run_bench(monkeypatch, capsys, "--dump-outputs", str(again))
    np.testing.assert_array_equal(np.load(again / "clip_embeddings.npy"), emb)


def test_full_run_adds_roofline_leg(monkeypatch, capsys):
    out = run_bench(monkeypatch, capsys, "--full", "--skip-cpu-baseline")
    assert out["ms_per_step"] > 0
    assert out["cpu_baseline"] is None  # skipped on request
    roof = out["roofline"]
    assert roof["kernel"] == "gemm_bf16" and roof["launches"] > 0
    assert 0.0 < roof["frac"] < 1.0
