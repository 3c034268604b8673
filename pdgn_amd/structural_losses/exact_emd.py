"""Exact EMD between clouds of equal size: the integer auction of csrc/auction.hip.  The reference has
no counterpart (its EMD is approxmatch, match_cost.py here); the cost is the same quantity -- the sum of Euclidean distances
over the matching -- with the matching a permutation and, at status 0, an optimum of the quantised problem."""

import torch
from .._fn import Function

from .. import _lib
from .._lib import check, ptr, require, stream_of

F32, I32 = torch.float32, torch.int32


def _pair(seta, setb):
    if torch.is_tensor(seta) and torch.is_tensor(setb) and seta.dim() == 3 and setb.dim() == 3 and seta.shape[1] != setb.shape[1]:
        raise ValueError("the exact EMD matches clouds of equal size (got %d and %d points): match_cost is the tool for unequal ones"
                         % (seta.shape[1], setb.shape[1]))
    require(seta, "seta", F32, 3)
    require(setb, "setb", F32, 3)
    if seta.shape[0] != setb.shape[0] or seta.shape[2] != 3 or setb.shape[2] != 3:
        raise ValueError("seta and setb must be (b,n,3) with one b, got %s and %s" % (tuple(seta.shape), tuple(setb.shape)))
    return seta.shape[0], seta.shape[1]


def auction_match(seta, setb, with_bids=False):
    """seta, setb (b,n,3) -> (assign (b,n) int32: point assign[p,i] of setb is matched to point i of seta; cost (b,): the fp32 sum
    of the matched distances; status (b,) int32: 0 optimal, 1 capped, 2 degenerate).  with_bids: also, fourth, the bids made (b,)
    int64."""
    b, n = _pair(seta, setb)
    dev = seta.device
    assign = torch.empty((b, n), dtype=I32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    status = torch.empty((b,), dtype=I32, device=dev)
    bids = torch.empty((b,), dtype=torch.int64, device=dev) if with_bids else None
    check(_lib.lib().pdgn_auction_assign(b, n, ptr(seta), ptr(setb), ptr(assign), ptr(cost), ptr(status), ptr(bids), stream_of(seta)),
          "pdgn_auction_assign")
    return (assign, cost, status, bids) if with_bids else (assign, cost, status)


class ExactEMDFunction(Function):
    """cost (b,) of the optimal assignment; the assignment is piecewise constant in the inputs, so the backward is the gradient of
    the matched distances at the assignment the forward found (pdgn_auction_cost_grad)."""

    @staticmethod
    def forward(ctx, seta, setb):
        assign, cost, _ = auction_match(seta, setb)
        ctx.save_for_backward(seta, setb, assign)
        return cost

    @staticmethod
    def backward(ctx, grad_output):
        seta, setb, assign = ctx.saved_tensors
        b, n = assign.shape
        g = grad_output.to(F32).contiguous()
        grada, gradb = torch.empty_like(seta), torch.empty_like(setb)
        check(_lib.lib().pdgn_auction_cost_grad(b, n, ptr(seta), ptr(setb), ptr(assign), ptr(g), ptr(grada), ptr(gradb), stream_of(seta)),
              "pdgn_auction_cost_grad")
        return grada, gradb


def exact_emd_cost(seta, setb):
    """match_cost's semantics on the exact matching: cost (b,).  The Function when a gradient is required, the plain launch otherwise."""
    if torch.is_grad_enabled() and (seta.requires_grad or setb.requires_grad):
        _pair(seta, setb)
        return ExactEMDFunction.apply(seta, setb)
    return auction_match(seta, setb)[1]
