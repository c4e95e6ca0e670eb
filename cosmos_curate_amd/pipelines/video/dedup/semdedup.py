"""Semantic dedup — multi-GPU k-means + pairwise max-cosine pruning.

Mirror of /root/reference/cosmos_curate/pipelines/video/dedup/
(dedup_pipeline.py:237 ``dedup``, dedup_actor.py ``SemDedupActor``
kmeans :182-313 / dedup :315-460, raft_actor.py NCCL wiring :84-132),
rebuilt MI355X-native (BASELINE config #5):

- the cuML ``KMeansMG`` fit over RAFT/NCCL becomes torch spherical
  k-means with ``torch.distributed`` all-reduce of centroid sums+counts
  over RCCL/xGMI (the same collective cuML issues per iteration); the
  unique-id broadcast dance of raft_actor.py:84-119 collapses into the
  process group init;
- the cuPy tiled strict-upper-triangular scan (dedup :393-460) becomes
  one HIP kernel on exact-f32 MFMA (csrc/cc_dedup.hip,
  ``cc_pairwise_max_earlier``), launched once a cluster, or with
  ``prune_backend="segmented"`` one launch sequence over all clusters
  (csrc/cc_dedupseg.hip, ``cc_pairwise_max_earlier_seg``);
- "kept" semantics identical: row pruned iff max-cosine to an earlier
  (farther-from-centroid) row exceeds 1 - eps.

No CPU fallback: ``pairwise_max_earlier`` requires the HIP extension +
GPU.  ``kmeans`` is plain torch by default and runs wherever its tensors
live — the world_size-2 gloo test drives the collective path on CPU; with
``backend="native"`` its assign and accumulate steps run on
csrc/cc_kmeans.hip (exact-f32 MFMA argmax, atomic-free f64 sums) and need
the GPU like the scan.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import torch

from cosmos_curate_amd import hotpath


@dataclasses.dataclass
class SemDedupConfig:
    """dedup_actor.py:47-74 subset."""

    n_clusters: int = 100
    n_iters: int = 20
    eps: float = 0.01
    random_seed: int = 0x5EED
    kmeans_backend: str = "torch"  # or "native": csrc/cc_kmeans.hip
    prune_backend: str = "loop"  # or "segmented": csrc/cc_dedupseg.hip


KMEANS_BACKENDS = ("torch", "native")
PRUNE_BACKENDS = ("loop", "segmented")


def _kmeans_operand(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-d float32 tensor")
    if not t.is_cuda:  # the kernels take device pointers only
        raise hotpath.HotpathUnavailableError(
            f"{name} must be a device tensor: the native k-means step has no CPU path")
    return t.contiguous()


def kmeans_assign(e: torch.Tensor, cent: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """labels[i] = argmax_c e_i . cent_c on the exact-f32 MFMA
    (cc_kmeans_assign), the smallest c among equal dot products; the [m, k]
    similarities are never stored.

    e (m, d) and cent (k, d) f32 device tensors, d a multiple of 64 in
    [64, 1152].  Returns (labels int64 [m], best f32 [m] = the winning dot
    product).  No fallback: a shape the kernel refuses raises."""
    lib = hotpath.require_gpu()
    e, cent = _kmeans_operand(e, "e"), _kmeans_operand(cent, "cent")
    (m, d), k = e.shape, cent.shape[0]
    if cent.shape[1] != d:
        raise ValueError(f"cent has {cent.shape[1]} columns, e has {d}")
    labels = torch.empty(m, dtype=torch.int32, device=e.device)
    best = torch.empty(m, dtype=torch.float32, device=e.device)
    stream = torch.cuda.current_stream(e.device).cuda_stream
    hotpath.check(lib.cc_kmeans_assign(
        e.data_ptr(), m, d, cent.data_ptr(), k, labels.data_ptr(),
        best.data_ptr(), stream))
    return labels.long(), best


def kmeans_accumulate(
    e: torch.Tensor, labels: torch.Tensor, k: int
) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-cluster f64 row sums and counts (cc_kmeans_accumulate): the
    index_add_ of the torch loop without floating-point atomics, so two calls
    on the same input agree bit for bit.

    e (m, d) f32 device tensor, labels integer [m] with values in [0, k).
    The stable sort of the labels and the clusters' offsets into it are
    torch integer plumbing (sort, searchsorted) that never synchronises with
    the host.  Returns (sums f64 [k, d], counts f64 [k]).  No fallback."""
    lib = hotpath.require_gpu()
    e = _kmeans_operand(e, "e")
    m, d = e.shape
    if labels.shape != (m,) or labels.device != e.device:
        raise ValueError("labels must be [m] on e's device")
    ws_bytes = lib.cc_kmeans_workspace_bytes(m, d, k)
    if ws_bytes < 0:
        hotpath.check(ws_bytes)
    sorted_labels, order = torch.sort(labels, stable=True)
    offsets = torch.searchsorted(
        sorted_labels, torch.arange(k + 1, dtype=labels.dtype, device=e.device)
    ).to(torch.int32)
    order = order.to(torch.int32)
    sums = torch.empty((k, d), dtype=torch.float64, device=e.device)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=e.device)
    stream = torch.cuda.current_stream(e.device).cuda_stream
    hotpath.check(lib.cc_kmeans_accumulate(
        e.data_ptr(), m, d, order.data_ptr(), offsets.data_ptr(), k,
        sums.data_ptr(), ws.data_ptr(), ws_bytes, stream))
    return sums, (offsets[1:] - offsets[:-1]).to(torch.float64)


def kmeans_fit(
    emb: torch.Tensor,
    n_clusters: int,
    n_iters: int = 20,
    seed: int = 0x5EED,
    process_group=None,
    backend: str = "torch",
) -> tuple[torch.Tensor, torch.Tensor]:
    """Spherical k-means over (possibly rank-sharded) embeddings.

    Each rank holds a shard; per iteration, assignment is local and the
    centroid sums/counts are all-reduced (the KMeansMG collective,
    dedup_actor.py:197-232).  Deterministic: init centroids are sampled
    by the shared seed from rank 0's shard size convention — all ranks
    compute the same init when fed identical full data (single rank) or
    receive rank-0's init via broadcast (multi rank).

    ``backend="native"`` runs assignment and the per-cluster sums on the HIP
    kernels (kmeans_assign, kmeans_accumulate) and needs device tensors and
    a ``d`` they take; it raises otherwise, it never falls back.  Init,
    broadcast, all-reduce and the normalise tail are shared.

    Returns (centroids [k,d] unit rows, local labels [m]).
    """
    if backend not in KMEANS_BACKENDS:
        raise ValueError(f"backend must be one of {KMEANS_BACKENDS}, got {backend!r}")
    e = torch.nn.functional.normalize(emb.float(), dim=1, eps=1e-12)
    m, d = e.shape
    dist = torch.distributed if process_group is not None else None

    rng = np.random.default_rng(seed)
    if dist is None or dist.get_rank(process_group) == 0:
        init_idx = np.sort(rng.choice(m, size=n_clusters, replace=False))
        cent = e[torch.from_numpy(init_idx.astype(np.int64))].clone()
    else:
        cent = torch.empty((n_clusters, d), dtype=e.dtype, device=e.device)
    if dist is not None:
        dist.broadcast(cent, src=0, group=process_group)

    labels = torch.zeros(m, dtype=torch.int64, device=e.device)
    for _ in range(n_iters):
        if backend == "native":
            labels, _ = kmeans_assign(e, cent)
            sums, counts = kmeans_accumulate(e, labels, n_clusters)
        else:
            sims = e @ cent.T
            labels = sims.argmax(dim=1)
            sums = torch.zeros((n_clusters, d), dtype=torch.float64, device=e.device)
            counts = torch.zeros(n_clusters, dtype=torch.float64, device=e.device)
            sums.index_add_(0, labels, e.to(torch.float64))
            counts.index_add_(0, labels, torch.ones_like(labels, dtype=torch.float64))
        if dist is not None:  # the RCCL all-reduce (dedup_actor.py:197-232)
            dist.all_reduce(sums, group=process_group)
            dist.all_reduce(counts, group=process_group)
        nz = counts > 0
        new = (sums[nz] / counts[nz, None]).to(e.dtype)
        cent[nz] = torch.nn.functional.normalize(new, dim=1, eps=1e-12)
    return cent, labels


def pairwise_max_earlier(
    e_sorted_dev: torch.Tensor,
) -> tuple[torch.Tensor, torch.Tensor]:
    """HIP strict-upper-triangular max-cosine scan (cc_pairwise_max_earlier).

    e_sorted_dev: (m, d) f32 CUDA tensor in scan order (L2-normalization is
    applied here, matching dedup_actor.py:399-407).  Returns
    (maxv f32 [m], argi i32 [m]) on device.
    """
    lib = hotpath.require_gpu()
    e = torch.nn.functional.normalize(e_sorted_dev.float(), dim=1, eps=1e-12).contiguous()
    m, d = e.shape
    maxv = torch.empty(m, dtype=torch.float32, device=e.device)
    argi = torch.empty(m, dtype=torch.int32, device=e.device)
    stream = torch.cuda.current_stream(e.device).cuda_stream
    hotpath.check(
        lib.cc_pairwise_max_earlier(e.data_ptr(), m, d, maxv.data_ptr(), argi.data_ptr(), stream)
    )
    return maxv, argi


def dedup_cluster(
    emb_sorted: torch.Tensor, eps: float
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One cluster's pruning pass (dedup_actor.py:315-460 semantics).

    Returns (kept_mask bool [m], maxv, argi).  Row kept iff
    max-cosine <= 1 - eps.
    """
    maxv, argi = pairwise_max_earlier(emb_sorted)
    kept = maxv <= (1.0 - eps)
    return kept, maxv, argi


def pairwise_max_earlier_segmented(
    e: torch.Tensor,
    order: torch.Tensor,
    offsets: torch.Tensor,
    *,
    seg_first: int = 0,
    seg_step: int = 1,
    out: tuple[torch.Tensor, torch.Tensor] | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """The pruning scan of every segment in one launch sequence
    (cc_pairwise_max_earlier_seg): no gathered copy of e, no host work per
    segment, no synchronisation.

    e (m, d) f32 device tensor of unit rows in their original order, d a
    multiple of 64 in [64, 1152]; order int32 [m], scan position -> row of e;
    offsets int32 [k+1], segment c = positions [offsets[c], offsets[c+1]).
    Only segments c with c % seg_step == seg_first are scanned.  Returns
    (maxv f32 [m], argi int32 [m]) indexed by scan position: the largest dot
    product with an earlier position of the same segment and that position
    within the segment, the smallest among equals; a segment's first position
    gets (0.0, 0).  Positions of other segments are not written: they keep
    what ``out`` (maxv, argi) held, or are uninitialised.  No fallback: a
    shape the kernel refuses raises."""
    lib = hotpath.require_gpu()
    e = _kmeans_operand(e, "e")
    m, d = e.shape
    k = offsets.numel() - 1
    for t, name, n in ((order, "order", m), (offsets, "offsets", k + 1)):
        if (t.dtype != torch.int32 or t.shape != (n,) or t.device != e.device
                or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 [{n}] tensor on e's device")
    ws_bytes = lib.cc_pairwise_seg_workspace_bytes(m, d, k)
    if ws_bytes < 0:
        hotpath.check(ws_bytes)
    if out is None:
        out = (torch.empty(m, dtype=torch.float32, device=e.device),
               torch.empty(m, dtype=torch.int32, device=e.device))
    maxv, argi = out
    if (maxv.dtype != torch.float32 or argi.dtype != torch.int32
            or maxv.shape != (m,) or argi.shape != (m,) or maxv.device != e.device
            or argi.device != e.device):
        raise ValueError("out must be (f32 [m], int32 [m]) on e's device")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=e.device)
    stream = torch.cuda.current_stream(e.device).cuda_stream
    hotpath.check(lib.cc_pairwise_max_earlier_seg(
        e.data_ptr(), m, d, order.data_ptr(), offsets.data_ptr(), k, seg_first,
        seg_step, maxv.data_ptr(), argi.data_ptr(), ws.data_ptr(), ws_bytes,
        stream))
    return maxv, argi


def prune_clusters(
    e: torch.Tensor,
    labels: torch.Tensor,
    dist_to_cent: torch.Tensor,
    k: int,
    eps: float,
    rank: int = 0,
    world: int = 1,
) -> tuple[torch.Tensor, torch.Tensor]:
    """The pruning pass over all clusters c with c % world == rank at once.

    The scan order is the per-cluster loop's: inside a cluster, farthest from
    the centroid first, equal distances in row order (two stable sorts, by
    distance descending then by label), and ``searchsorted`` finds the
    clusters' offsets: torch integer plumbing that never synchronises with
    the host.  e (m, d) unit rows on the device.  Returns (keep bool [m] in row
    order, True for rows of clusters this rank does not own; counts int64 [2] =
    kept and total rows of the owned clusters, still on the device)."""
    by_dist = torch.argsort(dist_to_cent, descending=True, stable=True)
    sorted_labels, by_label = torch.sort(labels[by_dist], stable=True)
    order = by_dist[by_label]
    offsets = torch.searchsorted(
        sorted_labels, torch.arange(k + 1, dtype=labels.dtype, device=e.device))
    maxv, _ = pairwise_max_earlier_segmented(
        e, order.to(torch.int32), offsets.to(torch.int32),
        seg_first=rank, seg_step=world)
    owned = sorted_labels % world == rank
    kept = (maxv <= (1.0 - eps)) & owned  # maxv is uninitialised elsewhere
    keep = torch.empty(len(e), dtype=torch.bool, device=e.device)
    keep[order] = kept | ~owned
    return keep, torch.stack([kept.sum(), owned.sum()])


def combine_keep_masks(keep: torch.Tensor, process_group=None) -> torch.Tensor:
    """AND the per-rank keep masks (each rank pruned only the clusters it
    owns, leaving the rest True) — the dedup_pipeline.py N>1 combine,
    RCCL MIN all-reduce on GPU ranks / gloo in the CPU tests."""
    if process_group is None:
        return keep
    ki = keep.int()
    torch.distributed.all_reduce(ki, op=torch.distributed.ReduceOp.MIN,
                                 group=process_group)
    return ki.bool()


def semdedup(
    embeddings: torch.Tensor,
    config: SemDedupConfig,
    process_group=None,
) -> dict:
    """Full pipeline for one rank's shard: k-means -> per-cluster pruning.

    Clusters are processed round-robin by rank (dedup_pipeline.py:237-300
    assigns cluster ranges to actors).  Returns counts + per-row keep mask
    aligned with the input order.

    ``config.prune_backend="segmented"`` prunes all of the rank's clusters in
    one launch sequence (prune_clusters) and synchronises once, for the two
    counts; ``"loop"`` launches the scan once a cluster.
    """
    if config.prune_backend not in PRUNE_BACKENDS:
        raise ValueError(
            f"prune_backend must be one of {PRUNE_BACKENDS}, got {config.prune_backend!r}")
    cent, labels = kmeans_fit(
        embeddings, config.n_clusters, config.n_iters, config.random_seed,
        process_group, backend=config.kmeans_backend,
    )
    e = torch.nn.functional.normalize(embeddings.float(), dim=1, eps=1e-12)
    cos_to_cent = (e * cent[labels]).sum(dim=1)
    dist_to_cent = 1.0 - cos_to_cent

    keep = torch.ones(len(e), dtype=torch.bool, device=e.device)
    rank = torch.distributed.get_rank(process_group) if process_group else 0
    world = torch.distributed.get_world_size(process_group) if process_group else 1
    if config.prune_backend == "segmented":
        keep, counts = prune_clusters(
            e, labels, dist_to_cent, config.n_clusters, config.eps, rank, world)
        kept_n, total_n = counts.tolist()
        return {"kept": kept_n, "total": total_n, "keep_mask": keep, "labels": labels}
    kept_n = 0
    total_n = 0
    for cid in range(rank, config.n_clusters, world):
        sel = (labels == cid).nonzero(as_tuple=True)[0]
        if len(sel) == 0:
            continue
        order = torch.argsort(dist_to_cent[sel], descending=True, stable=True)
        rows = sel[order]
        kept_mask, _, _ = dedup_cluster(e[rows], config.eps)
        keep[rows] = kept_mask
        kept_n += int(kept_mask.sum().item())
        total_n += len(rows)
    return {"kept": kept_n, "total": total_n, "keep_mask": keep, "labels": labels}
