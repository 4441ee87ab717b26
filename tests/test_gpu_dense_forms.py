"""The element kernels of csrc/dense.hip are one grid-stride map kernel with a functor per entry point, launched through one host-side
check. Pinned here for every entry point of the file, on the shapes and launchers of tools/dense_digest.py (B = 2, 3 x 5 maps of 8
channels; pooling to 1, 2 and 3 bins, 2 on 3 rows overlapping; resize to 7 x 4 and to 3 x 5 itself):

  - the launch that reads a column slice of a wider buffer and writes one equals the contiguous launch bit for bit, for float32 and
    bfloat16 on either side, and leaves every element outside its slice as it was;
  - the contiguous float32 result agrees with tests/dense_truth.py in float64 under the float32 rule of tests/test_gpu_dense_heads.py;
  - a cast-copy of 8200 x 520 elements, more than the 16384 x 256 threads of a launch so that the loop wraps, equals x.to(dtype)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import dense_truth as dtr
from test_gpu_dense_heads import close_f32, tok

pytestmark = pytest.mark.gpu


CASES = ([("evp_im2col3x3", {}), ("evp_col2im3x3", {})] +
         [(e, dict(s=s)) for e in ("evp_adaptive_avgpool_fwd", "evp_adaptive_avgpool_bwd") for s in (1, 2, 3)] +
         [(e, dict(size=z)) for e in ("evp_upsample_bilinear_fwd", "evp_upsample_bilinear_bwd") for z in ((7, 4), (3, 5))] +
         [("evp_channel_scale", dict(table=t)) for t in (True, False)] +
         [(e, dict(relu=r)) for e in ("evp_batchnorm_eval", "evp_batchnorm_eval_bwd") for r in (0, 1)] + [("evp_colsum_ordered", {})])


def _id(case):
    return case[0][4:] + "".join(f"-{k}{v}" for k, v in case[1].items()).replace(" ", "")


def frame(t, h, w):
    """token-major [B*h*w, C] -> (B, C, h, w)."""
    return t.reshape(-1, h, w, t.shape[1]).permute(0, 3, 1, 2)


def adjoint(fn, shape, g):
    """d/dx of (fn(x) * g).sum() at a float64 x of `shape`, token-major."""
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    (fn(x) * g.double()).sum().backward()
    return tok(x.grad)


def truth(entry, kw, p):
    from tools.dense_digest import B, C, EPS, H, W
    x = p["x"].double()
    if entry == "evp_im2col3x3":
        return dtr.im2col3x3(frame(x, H, W))
    if entry == "evp_col2im3x3":
        return adjoint(dtr.im2col3x3, (B, C, H, W), x)
    if entry == "evp_adaptive_avgpool_fwd":
        return tok(dtr.pool2d(frame(x, H, W), kw["s"]))
    if entry == "evp_adaptive_avgpool_bwd":
        return adjoint(lambda t: dtr.pool2d(t, kw["s"]), (B, C, H, W), frame(x, kw["s"], kw["s"]))
    if entry == "evp_upsample_bilinear_fwd":
        return tok(dtr.resize(frame(x, H, W), kw["size"]))
    if entry == "evp_upsample_bilinear_bwd":
        return adjoint(lambda t: dtr.resize(t, kw["size"]), (B, C, H, W), frame(x, *kw["size"]))
    if entry == "evp_channel_scale":
        return (x.view(B, H * W, C) * p["m"].double()[:, None, :]).view(-1, C) if kw["table"] else x
    if entry == "evp_batchnorm_eval":
        y = F.batch_norm(x, p["rm"].double(), p["rv"].double(), p["gamma"].double(), p["beta"].double(), False, 0.1, EPS)
        return F.relu(y) if kw["relu"] else y
    if entry == "evp_batchnorm_eval_bwd":
        dx = x * p["gamma"].double() / torch.sqrt(p["rv"].double() + EPS)
        return dx * (p["y"] > 0) if kw["relu"] else dx
    assert entry == "evp_colsum_ordered"
    return x.sum(0, keepdim=True)


def test_cases_are_the_tools_and_cover_every_entry_point_of_dense_hip():
    import os
    import re
    from eventpretrain_amd import _lib
    from tools.dense_digest import B, C, H, W, map_cases
    assert CASES == map_cases() and (B, H, W, C) == (2, 3, 5, 8)
    with open(os.path.join(_lib.CSRC, "dense.hip")) as f:
        assert set(re.findall(r'extern "C" int (evp_\w+)\(', f.read())) == {e for e, _ in CASES}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_strided_launch_is_the_contiguous_launch_and_stays_in_its_slice(case):
    from tools.dense_digest import FILL, map_launch, map_operands
    entry, kw = case
    p = map_operands(entry, kw)
    outs = (torch.float32,) if entry == "evp_colsum_ordered" else (torch.float32, torch.bfloat16)
    for ind, outd in itertools.product((torch.float32, torch.bfloat16), outs):
        _, flat = map_launch(entry, kw, p, ind, outd, strided=False)
        buf, view = map_launch(entry, kw, p, ind, outd, strided=True)
        torch.cuda.synchronize()
        assert flat.is_contiguous() and not (view.shape[0] > 1 and view.is_contiguous())
        assert torch.equal(flat.view(torch.uint8), view.contiguous().view(torch.uint8)), (entry, kw, ind, outd)
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:, view.storage_offset():view.storage_offset() + view.shape[1]] = False
        assert int(outside.sum()) == buf.numel() - view.numel() and bool((buf[outside] == FILL).all()), (entry, kw, ind, outd)
        assert not bool((flat == FILL).all())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_contiguous_f32_launch_matches_truth(case):
    from tools.dense_digest import map_launch, map_operands
    entry, kw = case
    p = map_operands(entry, kw)
    _, got = map_launch(entry, kw, p)
    torch.cuda.synchronize()
    close_f32(got, truth(entry, kw, p), _id(case))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_cast_copy_past_one_grid_of_threads(dtype):
    from tools.dense_digest import WRAP, wrap_launch, wrap_operand
    assert WRAP[0] * WRAP[1] > 16384 * 256
    x = wrap_operand()
    got = wrap_launch(x, dtype)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), x.to(dtype))
