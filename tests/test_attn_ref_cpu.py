"""The attention checker of attn_ref.py, proven without a GPU: over every
problem of the GPU grid the plain emulation of the kernels' numerics sits
within BOUND/3 of the float64 reference, and each wrong variant lands
beyond 2 x BOUND on the family that is responsible for it.  So a kernel
within BOUND (test_gpu_attn_scores.py) has none of these defects.
"""

import pytest
import torch

import attn_ref as R


@pytest.fixture(scope="module")
def measured():
    """One pass over PROBLEMS: {problem: (emulation errors, {variant: error})}."""
    out = {}
    for family, seq, hd in R.PROBLEMS:
        q, k, v = R.make_inputs(family, seq, hd, R.seed_of(family, seq, hd))
        ref = R.ref64(q, k, v)
        emu = {mode: R.error(R.emulate(q, k, v, mode), ref, v) for mode in (True, False)}
        wrong = {name: R.error(fn(q, k, v), ref, v)
                 for name, (fn, families, applies) in R.WRONG.items()
                 if family in families and applies(seq)}
        out[family, seq, hd] = (emu, wrong)
    return out


def test_grid_is_the_one_the_bound_was_measured_on():
    assert len(R.PROBLEMS) == 205 and len(R.GRID) == 302
    assert {f for f, _, _ in R.PROBLEMS} == set(R.FAMILIES)
    rungs = {}
    for rung, seq, hd, _ in R.GRID:
        rungs.setdefault(rung, set()).add((seq, hd))
    assert {r: len(s) for r, s in rungs.items()} == {
        "small": 9, "mid": 9, "flash": 15, "planned": 18, "cls": 5}


def test_emulation_within_a_third_of_the_bound(measured):
    worst = max((e, mode, p) for p, (emu, _) in measured.items() for mode, e in emu.items())
    print(f"worst emulation error {worst[0]:.6f} at {worst[2]} "
          f"({'normalised' if worst[1] else 'unnormalised'} P); BOUND {R.BOUND}")
    for mode in (True, False):
        print(f"  {'normalised' if mode else 'unnormalised'} P: worst "
              f"{max(emu[mode] for emu, _ in measured.values()):.6f}")
    assert worst[0] <= R.BOUND / 3
    # BOUND is 3 x the measured worst, not more
    assert R.BOUND <= 3 * worst[0] * 1.001


def test_every_wrong_variant_has_a_family():
    wrong_fns = {name for name in dir(R) if name.startswith("wrong_")}
    assert wrong_fns == {fn.__name__ for fn, _, _ in R.WRONG.values()}
    assert len(R.WRONG) == 8
    for name, (_, families, applies) in R.WRONG.items():
        assert families and set(families) <= set(R.FAMILIES), name
        hit = [p for p in R.PROBLEMS if p[0] in families and applies(p[1])]
        assert hit, f"{name}: no problem of the grid exposes it"
    # where the conditions start
    assert not R.WRONG["no_rescale"][2](64) and R.WRONG["no_rescale"][2](65)
    assert not R.WRONG["drop_last"][2](1) and R.WRONG["drop_last"][2](2)
    assert not R.WRONG["drop_last16"][2](1) and R.WRONG["drop_last16"][2](2)
    assert not R.WRONG["scale_x1.05"][2](32) and R.WRONG["scale_x1.05"][2](33)
    assert R.WRONG["one_zero_key"][2](1)


@pytest.mark.parametrize("name", list(R.WRONG))
def test_wrong_variant_is_caught(measured, name):
    errs = {p: wrong[name] for p, (_, wrong) in measured.items() if name in wrong}
    assert errs
    p = min(errs, key=errs.get)
    print(f"{name}: smallest error {errs[p]:.4f} at {p}, over {len(errs)} problems; "
          f"2 x BOUND {2 * R.BOUND:.5f}")
    for p, e in errs.items():
        assert e > 2 * R.BOUND, (name, p, e)


def test_zero_q_is_the_mean_of_v():
    for family, seq, hd in R.PROBLEMS:
        if family != "zero_q":
            continue
        q, k, v = R.make_inputs(family, seq, hd, R.seed_of(family, seq, hd))
        assert not q.any()
        want = v.double().mean(2, keepdim=True).expand(-1, -1, seq, -1)
        assert (R.ref64(q, k, v) - want).abs().max().item() <= 1e-12


def test_families_are_deterministic_and_shaped():
    for family in R.FAMILIES:
        a = R.make_inputs(family, 65, 72, 5)
        b = R.make_inputs(family, 65, 72, 5)
        for x, y in zip(a, b):
            assert x.dtype == torch.bfloat16 and x.shape == (R.N, R.HEADS, 65, 72)
            assert torch.equal(x, y)
    q, k, v = R.make_inputs("last_key", 65, 72, 5)
    assert (v[:, :, -1] == 4).all()
    # the fused layout round-trips
    qkv = R.fuse_qkv(q, k, v).reshape(R.N, 65, 3, R.HEADS, 72)
    assert torch.equal(qkv[:, :, 1].permute(0, 2, 1, 3), k)
    assert torch.equal(R.unfuse_out(R.fuse_qkv(q, k, v)[:, :R.HEADS * 72],
                                    R.N, R.HEADS, 65, 72), q)


def test_old_inputs_pass_wrong_attention():
    """The finding these tests start from, on the very inputs of
    test_gpu_iv2_kernels.py::test_attn_hd88_16_heads at seq 1025 (0.5 randn,
    2 frames, 16 heads of 88) under its assertion, rtol = atol = 2e-2
    against f32 sdpa: attention that drops the last 16 keys passes, attention
    that leaves 63 zero pad keys unmasked passes, and attention without any
    softmax (the mean of V) is within the tolerance at all but 7 of its 2.9
    million outputs (largest difference 0.0225).  The tolerance is larger than
    the output: its standard deviation is 0.016."""
    n, heads, hd, seq = 2, 16, 88, 1025
    q, k, v = R.old_inputs(n, heads, seq, hd, seed=1000 * hd + seq)
    sdpa = torch.nn.functional.scaled_dot_product_attention
    want = sdpa(q.float(), k.float(), v.float(), scale=R.scale_of(hd))
    assert want.std() < 2e-2

    torch.testing.assert_close(R.wrong_drop_last16(q, k, v).float(), want,
                               rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(R.wrong_zero_pad64(q, k, v).float(), want,
                               rtol=2e-2, atol=2e-2)
    mean_v = R.wrong_mean_v(q, k, v).float()
    diff = (mean_v - want).abs()
    outside = int((diff > 2e-2 + 2e-2 * want.abs()).sum())
    print(f"old inputs, mean of V vs f32 sdpa: max abs {diff.max():.4f}, {outside} of "
          f"{diff.numel()} outside the tolerance; std of the output {want.std():.4f}")
    assert outside <= 1e-5 * diff.numel() and diff.max() < 0.025

    # the same defects on a family of this module, under its metric
    q, k, v = R.make_inputs("neg_offset", seq, hd, 1)
    ref = R.ref64(q, k, v)
    assert R.error(R.wrong_mean_v(q, k, v), ref, v) > 2 * R.BOUND
    assert R.error(R.wrong_zero_pad64(q, k, v), ref, v) > 2 * R.BOUND
