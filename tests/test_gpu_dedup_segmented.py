"""The segmented pruning scan (csrc/cc_dedupseg.hip) against float64 on MI355X."""

import functools

import numpy as np
import pytest
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.pipelines.video.dedup import semdedup as sd
from oracle import semdedup as osd

pytestmark = pytest.mark.gpu

# a single j-tile is cut into chunks once its segment is longer than C i-tiles
C_TILES = 8  # the plan's chunk cap at these sizes, asserted in _run
LONG = C_TILES * 128 + 128 + 37  # C i-tiles, one more, and a partial tile


def _reference(e, order, lengths):
    """Per segment, in float64: normalise, E @ E.T, strict lower mask,
    first-occurrence argmax.  Returns (maxv, argi, gap between the top two)."""
    m = len(order)
    maxv, argi, gap = np.zeros(m), np.zeros(m, dtype=np.int64), np.full(m, np.inf)
    a = 0
    for n in lengths:
        seg = e[order[a:a + n]].astype(np.float64)
        seg /= np.linalg.norm(seg, axis=1, keepdims=True)
        s = seg @ seg.T
        s[np.triu_indices(n)] = -np.inf
        if n > 1:
            maxv[a + 1:a + n] = s[1:].max(axis=1)
            argi[a + 1:a + n] = s[1:].argmax(axis=1)
        if n > 2:
            top = np.partition(s[2:], -2, axis=1)[:, -2:]
            gap[a + 2:a + n] = top[:, 1] - top[:, 0]
        a += n
    return maxv, argi, gap


@functools.lru_cache(maxsize=None)
def _case(d, lengths, seed):
    """Random unit rows, a random permutation as the scan order, and the
    float64 reference, computed once."""
    rng = np.random.default_rng(seed)
    m = sum(lengths)
    e = osd.normalize_rows(rng.normal(size=(m, d)).astype(np.float32))
    order = rng.permutation(m).astype(np.int32)
    return e, order, _reference(e, order, lengths)


def _run(e, order, lengths, **kw):
    m, k = len(order), len(lengths)
    assert hotpath.pairwise_seg_plan(m, e.shape[1], k).chunk_tiles == C_TILES
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    args = [torch.from_numpy(x).cuda() for x in (e, order, offsets)]
    maxv, argi = sd.pairwise_max_earlier_segmented(*args, **kw)
    assert maxv.dtype == torch.float32 and argi.dtype == torch.int32
    return maxv, argi


@pytest.mark.parametrize(
    ("d", "lengths"),
    [(64, (1,)), (64, (63,)), (512, (64, 65)), (768, (0, 129, 0, 1, 0)),
     (1152, (5, LONG, 70)), (512, (2700, 0, 150, 100, 50))],  # 90 % in one segment
)
def test_segmented_vs_float64(d, lengths):
    e, order, (want_v, want_i, gap) = _case(d, lengths, seed=d + sum(lengths))
    maxv, argi = _run(e, order, lengths)
    again = _run(e, order, lengths)
    assert torch.equal(maxv, again[0]) and torch.equal(argi, again[1])
    maxv, argi = maxv.cpu().numpy(), argi.cpu().numpy()
    excused = argi != want_i
    print(f"segmented d {d} lengths {lengths}: max |maxv - f64| "
          f"{np.abs(maxv - want_v).max():.3g}, rows off the f64 argmax "
          f"{excused.sum()}, rows with gap < 1e-5 {(gap < 1e-5).sum()}")
    np.testing.assert_allclose(maxv, want_v, atol=2e-5, rtol=0)
    assert (gap[excused] < 1e-5).all()
    assert excused.sum() <= 0.005 * len(order)


def test_ties_across_chunks():
    """Exact copies of scan position 3 in a j-tile that is one item, in the
    first j-tile that is cut in two, and in the tile after it: every copy
    meets earlier copies in other i-chunks and must name the earliest."""
    lengths = (LONG,)
    e, order, _ = _case(64, lengths, seed=7)
    copies = [200, C_TILES * 128 + 5, C_TILES * 128 + 140]
    e = e.copy()
    e[order[copies]] = e[order[3]]
    maxv, argi = _run(e, order, lengths)
    np.testing.assert_array_equal(argi.cpu().numpy()[copies], 3)
    np.testing.assert_allclose(maxv.cpu().numpy()[copies], 1.0, atol=2e-5, rtol=0)


def test_ownership_leaves_other_segments_alone():
    lengths = (70, 130, 1, 40, 200)
    e, order, (want_v, want_i, gap) = _case(512, lengths, seed=11)
    m = len(order)
    out = (torch.full((m,), -7.0, device="cuda"),
           torch.full((m,), -7, dtype=torch.int32, device="cuda"))
    maxv, argi = _run(e, order, lengths, seg_first=1, seg_step=2, out=out)
    maxv, argi = maxv.cpu().numpy(), argi.cpu().numpy()
    owned = np.repeat(np.arange(5) % 2 == 1, lengths)
    assert (maxv[~owned] == -7.0).all() and (argi[~owned] == -7).all()
    np.testing.assert_allclose(maxv[owned], want_v[owned], atol=2e-5, rtol=0)
    off = owned & (argi != want_i)
    assert (gap[off] < 1e-5).all()


def test_semdedup_segmented_end_to_end(tmp_path):
    # the input of test_semdedup_end_to_end_gpu.  Every pruned row is an exact
    # copy and scores 1.0, every kept row scores far below 0.99 (random unit
    # rows in 512 dimensions), so the two kernels' different summation orders
    # cannot move a row across the threshold: the masks must be equal.
    rng = np.random.default_rng(1)
    base = osd.normalize_rows(rng.normal(size=(500, 512)).astype(np.float32))
    e = np.concatenate([base, base[rng.choice(500, size=120, replace=False)]])
    e = torch.from_numpy(e[rng.permutation(len(e))]).cuda()
    out = {b: sd.semdedup(e, sd.SemDedupConfig(n_clusters=8, n_iters=10, eps=0.01,
                                               prune_backend=b))
           for b in sd.PRUNE_BACKENDS}
    assert (out["segmented"]["total"], out["segmented"]["kept"]) == (len(e), len(e) - 120)
    assert torch.equal(out["segmented"]["keep_mask"], out["loop"]["keep_mask"])
    with pytest.raises(ValueError):
        sd.semdedup(e, sd.SemDedupConfig(prune_backend="batched"))

    # the input and the assertions of test_dedup_pipeline_cli
    import json

    import pyarrow as pa
    import pyarrow.parquet as pq

    from cosmos_curate_amd.pipelines.video.dedup_pipeline import cli_run_dedup

    rng = np.random.default_rng(12)
    m, d = 600, 512
    emb = rng.normal(size=(m, d)).astype(np.float32)
    emb[:60] = emb[60:120] + 0.001 * rng.normal(size=(60, d)).astype(np.float32)
    (tmp_path / "clip_embd").mkdir()
    pq.write_table(
        pa.table({"id": [f"c{i}" for i in range(m)], "embedding": [r for r in emb]}),
        tmp_path / "clip_embd" / "chunk_0.parquet")
    summary = cli_run_dedup([
        "--input-embeddings-path", str(tmp_path),
        "--output-dedup-path", str(tmp_path / "dedup"),
        "--n-clusters", "8", "--eps", "0.05", "--prune-backend", "segmented"])
    assert summary["num_embeddings"] == m
    assert summary["num_removed"] >= 55  # the planted near-dupes
    t = pq.read_table(tmp_path / "dedup" / "dedup_results.parquet")
    assert t.num_rows == m and set(t.column_names) == {"id", "cluster", "keep"}
    disk = json.loads((tmp_path / "dedup" / "summary.json").read_text())
    assert disk["num_kept"] == summary["num_kept"]
    assert disk["prune_backend"] == "segmented"
