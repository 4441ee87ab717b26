"""The side record of a residual-stream gradient (ops._side_put / ops._side_take) on the host, no GPU: it is an attribute on the
tensor that the LayerNorm backward made, so it reaches exactly the one autograd.Function that receives that tensor (or a whole view
of it) unchanged, and nobody else."""
import pytest
import torch

from eventpretrain_amd import ops

NONE = (None, None)


def _chain(as_view, second_use=False):
    """consumer(producer(x)) backward; the producer's backward (the consumer's neighbour BELOW, as a block's last LayerNorm backward
    is) puts a record on its fresh dx and returns it flat or as a view; -> (what the next backward took, what was put)."""
    put, took = {}, {}

    class Upper(torch.autograd.Function):           # receives the loss gradient, hands a recorded dx down
        @staticmethod
        def forward(ctx, x):
            return x * 2.0

        @staticmethod
        def backward(ctx, g):
            dx = torch.full((6, 4), 2.0)
            put["lp"], put["cs"] = dx.bfloat16(), dx.sum(0, keepdim=True)
            ops._side_put(dx, put["lp"], put["cs"])
            return dx.view(2, 3, 4) if as_view else dx

    class Lower(torch.autograd.Function):           # the block below: its incoming gradient is Upper's dx
        @staticmethod
        def forward(ctx, x):
            return x + 1.0

        @staticmethod
        def backward(ctx, g):
            took["g"] = g
            took["side"] = ops._side_take(g.contiguous().view(6, 4))
            return g

    x = torch.zeros(2, 3, 4, requires_grad=True) if as_view else torch.zeros(6, 4, requires_grad=True)
    h = Lower.apply(x)
    out = Upper.apply(h).sum()
    if second_use:
        out = out + (h * 3.0).sum()                 # h has two consumers: autograd sums their gradients before Lower.backward
    out.backward()
    return took, put


@pytest.mark.parametrize("as_view", [False, True])
def test_record_arrives_with_the_tensor(as_view):
    took, put = _chain(as_view)
    assert took["side"][0] is put["lp"] and took["side"][1] is put["cs"]


@pytest.mark.parametrize("as_view", [False, True])
def test_summed_gradient_carries_no_record(as_view):
    took, put = _chain(as_view, second_use=True)
    assert took["side"] == NONE
    assert torch.equal(took["g"].reshape(6, 4), torch.full((6, 4), 5.0))      # really the sum of both uses


def _recorded():
    dx = torch.zeros(6, 4)
    lp, cs = dx.bfloat16(), dx.sum(0, keepdim=True)
    ops._side_put(dx, lp, cs)
    return dx, lp, cs


def test_in_place_change_voids_the_record():
    dx, _, _ = _recorded()
    dx.add_(1)
    assert ops._side_take(dx) == NONE
    dx, _, _ = _recorded()
    dx.view(2, 3, 4).add_(1)                        # views share the version counter
    assert ops._side_take(dx.view(6, 4)) == NONE


def test_partial_view_gets_nothing():
    dx, _, _ = _recorded()
    part = dx[1:]
    assert part.is_contiguous() and part._base is dx
    assert ops._side_take(part) == NONE
    dx, _, _ = _recorded()
    assert ops._side_take(dx[:5]) == NONE           # same address, fewer elements
    dx, _, _ = _recorded()
    assert ops._side_take(dx.t()) == NONE           # whole but not contiguous


def test_record_is_taken_once_and_released():
    dx, lp, cs = _recorded()
    got = ops._side_take(dx.view(2, 3, 4))
    assert got[0] is lp and got[1] is cs
    assert ops._side_take(dx) == NONE and ops._side_take(dx.view(2, 3, 4)) == NONE
    assert not hasattr(dx, "_evp_side")             # the bf16 copy is not kept alive by the gradient tensor
    assert ops._side_take(torch.zeros(6, 4)) == NONE
