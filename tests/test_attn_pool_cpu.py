"""What cc_attn_pool rests on that needs no GPU: its launch plan, the two
folds of a pooling head into (U, pooled rows, V projection), held in float64
through attn_pool_ref to the heads as the towers' torch routes write them,
and the flag's refusal for a tower without a pooling head.
"""

import argparse

import pytest
import torch

import attn_pool_ref as R
from cosmos_curate_amd import build as cc_build
from cosmos_curate_amd import hotpath

CC_ERR_UNSUPPORTED = -6


@pytest.fixture(scope="module", autouse=True)
def lib():
    cc_build.build(verbose=False)
    return hotpath.load()


@pytest.mark.parametrize("n", [1, 8, 64, 300])
def test_plan_splits_cover_seq_exactly(n):
    for seq in range(1, 2050):
        p = hotpath.attn_pool_plan(n, seq, 16, 1408)
        tokens = p.chunk * p.chunks_per_split
        # the last split starts inside the sequence, all of them reach its end
        assert (p.splits - 1) * tokens < seq <= p.splits * tokens, (n, seq)
        assert p.grid == n * p.splits and p.block == 512
        assert p.workspace_floats == (
            0 if p.splits == 1 else n * p.splits * (48 + 16 * 1408))
    # an explicit split count is taken as given, empty splits included
    assert hotpath.attn_pool_plan(2, 33, 16, 1024, 3).splits == 3


@pytest.mark.parametrize("heads,H", [(17, 1152), (0, 1152), (16, 1536), (16, 1100), (16, 64)])
def test_plan_refuses_unsupported_geometry(lib, heads, H):
    assert not hotpath.attn_pool_supported(heads, H)
    plan = hotpath.AttnPoolPlan()
    assert lib.cc_attn_pool_plan(1, 1, heads, H, 0, plan) == CC_ERR_UNSUPPORTED
    assert all(hotpath.attn_pool_supported(16, w) for w in (1024, 1152, 1408))


def _head_inputs(seed, n=2, seq=37, heads=4, hd=6):
    H = heads * hd
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return n, seq, heads, hd, H, r


def _attend(q, k, v, n, heads, hd):
    k = k.reshape(n, -1, heads, hd).transpose(1, 2)
    v = v.reshape(n, -1, heads, hd).transpose(1, 2)
    att = torch.softmax(q.unsqueeze(2) @ k.transpose(-1, -2), dim=-1)
    return (att @ v).reshape(n, heads * hd)


def test_siglip_fold_reproduces_the_map_head_attention():
    from cosmos_curate_amd.models.siglip_vit import fold_map_probe

    n, seq, heads, hd, H, r = _head_inputs(1)
    x, probe, w, b = r(n, seq, H), r(1, 1, H), r(3 * H, H) / H ** 0.5, r(3 * H)
    (wq, wk, wv), (bq, bk, bv) = w.chunk(3), b.chunk(3)
    q = ((probe[0, 0] @ wq.T + bq) * hd ** -0.5).reshape(1, heads, hd).expand(n, -1, -1)
    want = _attend(q, x @ wk.T + bk, x @ wv.T + bv, n, heads, hd)

    u = fold_map_probe(probe, w, b, heads)
    zhat = R.zhat_ref(x, u[None], None, None)
    got = torch.einsum("nhk,hdk->nhd", zhat, wv.reshape(heads, hd, H)).reshape(n, H) + bv
    assert (got - want).abs().max() <= 1e-9


def test_internvideo2_fold_reproduces_the_clip_projector_attention():
    from cosmos_curate_amd.models.internvideo2_vit import fold_pool_head, pool_probe

    n, seq, heads, hd, H, r = _head_inputs(2)
    x, q = r(n, seq, H) + 2 * r(n, seq, 1), r(n, heads, hd)
    wk, wv, bk, bv = r(H, H) / H ** 0.5, r(H, H) / H ** 0.5, r(H), r(H)
    gk, gv, betak, betav = 1 + 0.2 * r(H), 1 + 0.2 * r(H), 0.1 * r(H), 0.1 * r(H)
    ln = lambda g, b_: torch.nn.functional.layer_norm(x, (H,), g, b_, eps=R.LN_EPS)  # noqa: E731
    want = _attend(q, ln(gk, betak) @ wk.T + bk, ln(gv, betav) @ wv.T + bv, n, heads, hd)

    uk, wvf, bvf = fold_pool_head(wk, gk, wv, bv, gv, betav, heads)
    mu = x.mean(dim=-1)
    rstd = torch.rsqrt(x.var(dim=-1, unbiased=False) + R.LN_EPS)
    zhat = R.zhat_ref(x, pool_probe(q, uk), mu, rstd)
    got = torch.einsum("nhk,hdk->nhd", zhat, wvf).reshape(n, H) + bvf
    assert (got - want).abs().max() <= 1e-9


def _assemble(argv):
    from cosmos_curate_amd.pipelines.video import splitting_pipeline as sp

    _assemble_stages, _setup_parser = sp._assemble_stages, sp._setup_parser
    p = argparse.ArgumentParser()
    _setup_parser(p)
    return _assemble_stages(p.parse_args(
        ["--input-video-path", "/in", "--output-clip-path", "/out", *argv]))


def test_cli_pool_head_flag():
    with pytest.raises(ValueError, match="attention-pooling head"):
        _assemble(["--embedding-pool-head", "native"])  # vit_b32: a CLIP tower
    for argv in (["--embedding-model", "siglip_so400m_14_224"],
                 ["--embedding-algorithm", "internvideo2"]):
        for pool in ("torch", "native"):
            stage = _assemble([*argv, "--embedding-pool-head", pool])[-2]
            assert getattr(stage, "stage", stage).model._pool_head == pool
