"""The truth of the dense-prediction heads (tests/dense_truth.py) on the host, no GPU: (1) the float64 restatement equals the reference's own
classes (tests/golden/ft_dense_heads.npz) to 1e-10; (2) pooling bins, bilinear taps and their adjoints against torch's functions; (3) the
comparator's input condition for every case the GPU test runs; (4) mutants of the restatement each fail the comparator."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_truth as dtr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ft_dense_heads.npz"))


def _conv_weight_of(bias_key):
    return bias_key[:-len("bias")] + "weight"


@pytest.mark.parametrize("head,shape,train", dtr.FIXTURE_CASES)
def test_restatement_equals_the_reference_heads(golden, head, shape, train):
    tag = f"{head}.{shape}.{'train' if train else 'eval'}"
    (case,) = [c for c in json.loads(str(golden["cases"])) if c["tag"] == tag]
    T, _ = dtr.reference(head, shape, train)
    assert sorted(case["tensors"]) == sorted(T)
    for k in case["tensors"]:
        t = T[k]
        if k.endswith("num_batches_tracked"):
            assert int(t.item()) == int(golden[f"{tag}|{k}"]) == (1 if train else 0), k
            continue
        if train and k.startswith("grad:") and dtr.is_prebn_bias(k):
            # zero up to rounding on both sides: compared absolutely, against the same convolution's weight gradient
            bound = 1e-9 * T[_conv_weight_of(k)].abs().max().item()
            assert t.abs().max().item() <= bound and np.abs(golden[f"{tag}|{k}"]).max() <= bound, k
            continue
        if t.numel() > dtr.BIG:
            ref = torch.from_numpy(golden[f"{tag}|{k}|sample"])
            assert dtr.rel_err(t.flatten()[::dtr.SAMPLE], ref) <= 1e-10, k
            got, want = dtr.checksums(t), torch.from_numpy(golden[f"{tag}|{k}|sums"])
            scale = torch.stack([want[1], want[1], want[1], want[3]])            # sums against sum |.|, squares against squares
            assert ((got - want).abs() <= 1e-10 * scale).all(), (k, got, want)
        else:
            ref = torch.from_numpy(golden[f"{tag}|{k}"])
            assert t.shape == ref.shape and dtr.rel_err(t, ref) <= 1e-10, k


@pytest.mark.parametrize("H,W,s", dtr.GEOMETRY)
def test_pool_bins_upsample_taps_and_their_adjoints(H, W, s):
    g = torch.Generator().manual_seed(H * 100 + W * 10 + s)
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=g)
    ph, pw = dtr.pool_matrix(H, s), dtr.pool_matrix(W, s)
    pooled = torch.einsum("ih,bchw,jw->bcij", ph, x, pw)
    assert torch.allclose(pooled, F.adaptive_avg_pool2d(x, s), rtol=1e-12, atol=1e-13)
    for n in (H, W):           # the bins are floor / ceil, and overlap exactly where s does not divide n
        bins = dtr.pool_bins(n, s)
        assert bins[0][0] == 0 and bins[-1][1] == n and all(b > a for a, b in bins)
        assert any(bins[i][1] > bins[i + 1][0] for i in range(s - 1)) == (n % s != 0 and s > 1)
    uh, uw = dtr.bilinear_matrix(s, H), dtr.bilinear_matrix(s, W)
    up = torch.einsum("hi,bcij,wj->bchw", uh, pooled, uw)
    assert torch.allclose(up, F.interpolate(pooled, size=(H, W), mode="bilinear", align_corners=False), rtol=1e-12, atol=1e-13)
    assert torch.allclose(uh.sum(1), torch.ones(H, dtype=torch.float64)) and (uh >= 0).all()
    # adjoints: <A x, y> = <x, A^T y>, A^T from the transposed matrices (what the gather kernels compute) and from autograd
    y = torch.randn(2, 3, H, W, dtype=torch.float64, generator=g)
    xr = x.clone().requires_grad_(True)
    a = F.interpolate(F.adaptive_avg_pool2d(xr, s), size=(H, W), mode="bilinear", align_corners=False)
    (a * y).sum().backward()
    aty = torch.einsum("ih,jw,bcij->bchw", ph, pw, torch.einsum("hi,wj,bchw->bcij", uh, uw, y))
    assert torch.allclose(aty, xr.grad, rtol=1e-12, atol=1e-13)
    assert (a.detach() * y).sum().item() == pytest.approx((x * aty).sum().item(), rel=1e-12)


def test_im2col_restatement_is_the_convolution():
    x = torch.randn(2, 8, 5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    w = torch.randn(6, 8, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    y = dtr.im2col3x3(x) @ w.view(6, 72).t()
    assert torch.allclose(y.view(2, 5, 7, 6).permute(0, 3, 1, 2), F.conv2d(x, w, padding=1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("head,shape,train,drop", dtr.BF16_CASES)
def test_comparator_input_condition(head, shape, train, drop):
    """The yardstick against truth passes its own gates (ratio <= 1 of FACTOR) and leaves at most MAX_EXCLUDED of any family out
    (asserted inside block_truth.compare), for every case of the GPU test: the GPU test cannot hide behind exclusions."""
    T, Y = dtr.reference(head, shape, train, drop)
    fails, worst = dtr.compare_case(Y, T, Y, train)
    assert not fails, fails
    assert worst and max(worst.values()) <= 1.0 + 1e-12
    f32 = dtr.run_head(head, shape, train, "f32", drop)
    assert all(dtr.rel_err(f32[k], T[k]) <= 1e-4 for k in worst), "float32 is not near float64 truth"


@pytest.mark.parametrize("mutant", dtr.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparator(mutant):
    head, shape, train, drop = dtr.MUTANT_CASE[mutant]
    T, Y = dtr.reference(head, shape, train, drop)
    got = dtr.run_head(head, shape, train, "truth", drop, mut=(mutant,))
    fails, _ = dtr.compare_case(got, T, Y, train)
    assert fails, f"{mutant} passes the comparator"
