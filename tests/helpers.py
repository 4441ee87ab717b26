"""Shared by CPU and GPU tests: checksum function (same definition as oracle/gen_golden.py), state-dict builders."""
import json

import numpy as np
import torch

from eventpretrain_amd.testing import det_uniform, det_value_for


def checksums(t: torch.Tensor):
    d = t.detach().double().flatten().cpu()
    w = det_uniform("checksum.weights", (d.numel(),)).double()
    return np.array([d.sum().item(), d.abs().sum().item(), (d * w).sum().item(), (d * d).sum().item()])


def assert_checksums(t, ref, rtol, what=""):
    got = checksums(t)
    scale = max(abs(ref[1]), 1e-30)          # sum |x| sets the scale for sum / weighted sum
    assert abs(got[0] - ref[0]) <= rtol * scale, (what, got, ref)
    assert abs(got[1] - ref[1]) <= rtol * scale, (what, got, ref)
    assert abs(got[2] - ref[2]) <= rtol * scale, (what, got, ref)
    assert abs(got[3] - ref[3]) <= 2 * rtol * max(abs(ref[3]), 1e-30), (what, got, ref)


def rec_state_dict(cfg):
    """State dict (reference key names) of the hand-composed ViT + PrRecDecoder with the
    closed-form fill; pos_embed tables come from the oracle's sincos restatement."""
    from oracle.model_oracle import sincos_2d
    D, Dd, p = cfg["dim"], cfg["dec_dim"], cfg["patch"]
    g = cfg["input"] // p
    L = g * g
    shapes = {"backbone.patch_embed.proj.weight": (D, 5, p, p), "backbone.patch_embed.proj.bias": (D,),
              "backbone.patch_embed.norm.weight": (D,), "backbone.patch_embed.norm.bias": (D,),
              "backbone.norm_layer.weight": (D,), "backbone.norm_layer.bias": (D,),
              "pretrain_rec_decoder.mask_token": (1, 1, Dd),
              "pretrain_rec_decoder.patch_embed.weight": (Dd, D), "pretrain_rec_decoder.patch_embed.bias": (Dd,),
              "pretrain_rec_decoder.norm.weight": (Dd,), "pretrain_rec_decoder.norm.bias": (Dd,),
              "pretrain_rec_decoder.pred.weight": (p * p, Dd), "pretrain_rec_decoder.pred.bias": (p * p,)}
    for pre, depth, d in (("backbone.vit_block.", cfg["depth"], D), ("pretrain_rec_decoder.vit_block.", cfg["dec_depth"], Dd)):
        for i in range(depth):
            b = f"{pre}{i}."
            shapes.update({b + "norm1.weight": (d,), b + "norm1.bias": (d,), b + "norm2.weight": (d,), b + "norm2.bias": (d,),
                           b + "attn.qkv.weight": (3 * d, d), b + "attn.qkv.bias": (3 * d,),
                           b + "attn.proj.weight": (d, d), b + "attn.proj.bias": (d,),
                           b + "mlp.fc1.weight": (4 * d, d), b + "mlp.fc1.bias": (4 * d,),
                           b + "mlp.fc2.weight": (d, 4 * d), b + "mlp.fc2.bias": (d,)})
    sd = {k: det_value_for(k, s) for k, s in shapes.items()}
    sd["backbone.pos_embed"] = torch.from_numpy(sincos_2d(D, g)).float().unsqueeze(0)
    sd["pretrain_rec_decoder.pos_embed"] = torch.from_numpy(sincos_2d(Dd, g)).float().unsqueeze(0)
    return sd


def rec_inputs(tag, cfg):
    from eventpretrain_amd.testing import det_normalish
    B, S = cfg["B"], cfg["input"]
    L = (S // cfg["patch"]) ** 2
    x = det_normalish(f"{tag}.voxels", (B, 5, S, S)) * 0.5
    y = det_normalish(f"{tag}.sub_frame", (B, 1, S, S))
    noise = det_uniform(f"{tag}.noise", (B, L), 0.0, 1.0)
    return x, y, noise


def jl(a):
    return json.loads(str(a))


# ----------------------------------------------------------------------------------------------- density masking
def density_inputs(d, tag):
    """Re-make the input grids of tests/golden/masking_density.npz bit for bit: clip cases go through the pinned CPU
    voxel oracle (bit-exact against the reference's events_to_voxel_grid), the random case through det_normalish. The
    fixture's checksums of the reference-made grids are asserted."""
    from eventpretrain_amd.testing import det_normalish, synthetic_events
    from oracle.voxel_oracle import voxel_grid
    spec = jl(d["inputs"])[tag]
    if spec["kind"] == "clips":
        gs = []
        for sd in spec["seeds"]:
            ev = synthetic_events(sd, spec["n_ev"])
            if spec["band"] is not None:
                ev = ev[~((ev[:, 1] >= spec["band"][0]) & (ev[:, 1] < spec["band"][1]))]
            gs.append(torch.from_numpy(voxel_grid(ev, 5, (224, 224))))
        x = torch.stack(gs).float()
    else:
        x = det_normalish(spec["name"], (spec["B"], 5, 224, 224)) * 0.5
    # (float64 sums of identical float32 data; only the summation order of torch.sum varies with the thread count)
    assert np.allclose(checksums(x), d[f"{tag}_x_checksums"], rtol=1e-12, atol=0), f"input grids of case {tag} differ from the fixture's"
    return x


def assert_ids_equal_up_to_ties(noise, keep, ref, got, what=""):
    """ref / got = (ids_keep, mask, ids_restore) as numpy. The order among EQUAL noise values is not a property of the
    reference's algorithm but of the sort routine torch picked (x86-simd-sort on the CPU build that made the fixture, a
    radix sort on CUDA): an implementation must (1) produce a valid ascending argsort, (2) agree with the reference on
    every token whose noise value is unique in its row -- rank, keep-membership and mask -- and (3) give each group of
    tied tokens the same SET of ranks. Rows without ties are therefore compared bit for bit."""
    noise = np.asarray(noise)
    B, L = noise.shape
    for name, (ids_keep, mask, restore) in (("reference", ref), ("implementation", got)):
        for b in range(B):
            assert sorted(restore[b].tolist()) == list(range(L)), (what, name, b, "ids_restore is not a permutation")
            order = np.argsort(restore[b], kind="stable")
            assert np.all(np.diff(noise[b][order]) >= 0), (what, name, b, "not an ascending argsort")
            assert np.array_equal(order[:keep], ids_keep[b]), (what, name, b, "ids_keep is not the head of the order")
            assert np.array_equal(mask[b], (restore[b] >= keep).astype(np.float32)), (what, name, b, "mask")
    for b in range(B):
        vals, inv, cnt = np.unique(noise[b], return_inverse=True, return_counts=True)
        uniq = cnt[inv] == 1
        assert np.array_equal(ref[2][b][uniq], got[2][b][uniq]), (what, b, "rank of a token with a unique noise value")
        assert np.array_equal(ref[1][b][uniq], got[1][b][uniq]), (what, b, "mask of a token with a unique noise value")
        for g in np.nonzero(cnt > 1)[0]:
            idx = np.nonzero(inv == g)[0]
            assert sorted(ref[2][b][idx].tolist()) == sorted(got[2][b][idx].tolist()), (what, b, "rank set of a tie group")
        if not (cnt > 1).any():
            for k in range(3):
                assert np.array_equal(ref[k][b], got[k][b]), (what, b, k)


# ----------------------------------------------------------------------------------------------- distribution checks
def normal_cdf(x):
    """Standard normal CDF, elementwise over a numpy array."""
    from math import erfc, sqrt
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * np.vectorize(erfc)(-x / sqrt(2.0))


def chi2_isf(p, dof):
    """Upper p-quantile of the chi-square distribution with `dof` degrees of freedom (Wilson-Hilferty; the normal quantile by
    bisection). Within a few per cent of the exact value for dof >= 3 and p >= 1e-9: enough for a p ~ 1e-6 test threshold."""
    from math import erfc, sqrt
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * erfc(mid / sqrt(2.0)) > p:
            lo = mid
        else:
            hi = mid
    z, k = 0.5 * (lo + hi), float(dof)
    return k * (1.0 - 2.0 / (9.0 * k) + z * sqrt(2.0 / (9.0 * k))) ** 3
