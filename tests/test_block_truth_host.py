"""The float64-truth gate of the bf16 blocks (tests/block_truth.py) on the host, no GPU: its references are sane for every case the
GPU tests run, and the comparator is neither vacuous nor blind -- it accepts the yardstick's own noise, also doubled, and rejects
each of a list of confined defects laid over that noise."""
import pytest
import torch

import block_truth as bt


def _noisy(ref, k=1.0):
    """Truth plus k times the yardstick's own error: what a correct bf16 implementation looks like to the comparator."""
    return {t: ref.T[t] + k * (ref.Y[t] - ref.T[t]) for t in ref.tensors}


def _check(name, got):
    ref = bt.reference(name)
    return bt.compare_all(got, ref, heads=bt.heads_of(name), blocks=name != "rec_tiny")[0]


@pytest.mark.parametrize("name", bt.CASES)
def test_references_are_sane(name):
    """e_ref > 0 for every tensor (there is a scale to measure with), the f32 oracle within 1e-5 relative of the float64 run (truth
    is truth), and truth itself keeps within the cap on left-out sub-blocks (compare() asserts the share for every family)."""
    ref = bt.reference(name)
    assert "dx" in ref.tensors or name == "rec_tiny"
    assert sum(t.startswith("grad:") for t in ref.tensors) == sum(p.requires_grad for p in bt.make_case(name)["module"].parameters()) \
        or name == "rec_tiny"
    for t in ref.tensors:
        assert torch.isfinite(ref.T[t]).all() and ref.T[t].norm() > 0, t
        assert ref.e_ref(t) > 0, t
        assert bt.rel_err(ref.F[t], ref.T[t]) <= 1e-5, (t, bt.rel_err(ref.F[t], ref.T[t]))
    assert _check(name, {t: ref.T[t] for t in ref.tensors}) == []
    if name == "rec_tiny":          # the three runs masked the same tokens, and every trainable parameter of the two towers has a gradient
        assert torch.equal(ref.T["_mask"], ref.Y["_mask"]) and torch.equal(ref.T["_ids_restore"], ref.F["_ids_restore"])
        assert len([t for t in ref.tensors if t.startswith("grad:")]) > 200


@pytest.mark.parametrize("name", bt.CASES)
def test_comparator_accepts_the_yardsticks_noise_and_twice_it(name):
    ref = bt.reference(name)
    assert _check(name, _noisy(ref)) == []
    assert _check(name, _noisy(ref, 2.0)) == []
    fails, worst, _ = bt.compare_all(_noisy(ref, 2.0), ref, heads=bt.heads_of(name), blocks=name != "rec_tiny")
    assert 1.9 < worst[0] <= 2.0 + 1e-9, worst


def _defects(name):
    """-> [(label, tensor that must be flagged, function changing the dict of tensors in place)]."""
    ref = bt.reference(name)
    c = bt.make_case(name)
    pre = "grad:0." if c["kind"] == "vit" else "grad:"
    out = []

    def two_d(t):
        return t.view(-1, t.shape[-1])

    if name != "rec_tiny":
        out.append(("dx: one 16 x 64 block zeroed", "dx", lambda g: two_d(g["dx"])[16:32, 0:64].zero_()))
        out.append(("dx: one 16-row strip doubled", "dx", lambda g: two_d(g["dx"])[32:48].mul_(2.0)))
        fc1 = pre + "mlp.fc1.weight"
        out.append(("fc1 weight gradient: one 128 x 128 block dropped", fc1, lambda g: g[fc1].view(g[fc1].shape[0], -1)[128:256, 0:128].zero_()))
    if c["kind"] in ("vit", "swin"):
        D, heads = c["spec"]["D"], c["spec"]["heads"]
        dh = D // heads
        qw, qb = pre + "attn.qkv.weight", pre + "attn.qkv.bias"

        def swap(g):
            k = g[qw][D:2 * D].clone()
            g[qw][D:2 * D] = g[qw][2 * D:]
            g[qw][2 * D:] = k
        out.append(("qkv weight gradient: k and v thirds swapped", qw, swap))
        out.append(("qkv bias gradient: one head's slice negated", qb, lambda g: g[qb][2 * D + dh:2 * D + 2 * dh].neg_()))
    for t in ref.tensors:
        out.append((f"{t}: scaled by 1 / 0.7", t, lambda g, t=t: g[t].div_(0.7)))
    norms = [t for t in ref.tensors if t.endswith(("norm1.weight", "norm2.weight", "norm.weight", "norm_layer.weight"))]
    for t in norms:
        b = t[:-len("weight")] + "bias"
        out.append((f"{t}: replaced by the norm-bias gradient", t, lambda g, t=t, b=b: g[t].copy_(g[b])))
    return out


@pytest.mark.parametrize("name", bt.CASES)
def test_comparator_rejects_confined_defects(name):
    """Each defect is laid over truth + the yardstick's noise (which the test above shows accepted): the comparator must flag the
    tensor it sits in."""
    ref = bt.reference(name)
    defects = _defects(name)
    assert len(defects) >= (6 if name != "rec_tiny" else 200)
    for label, tensor, apply in defects:
        got = {t: v.clone() for t, v in _noisy(ref).items()}
        apply(got)
        fails = _check(name, {tensor: got[tensor]})
        assert fails and all(f.startswith(tensor + "/") for f in fails), (label, fails)
