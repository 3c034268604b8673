"""CPU: the host side of the dense layers (pdgn_amd/fused.py).  The three hand-overs between autograd nodes -- zero column sums,
row maxima, carried input gradients -- through their public names: which tensor, presented later, still stands for the marked one
(the rules differ on purpose); and the route of a dense call on tensors that are not on the device."""
import pytest
import torch

from pdgn_amd import fused

CHANNELS = ("zero_colsum", "maxima", "input_grad")
PAYLOAD = object()


def _mark(channel, view=False):
    """A marked (6, 4) tensor; view: one that is itself a view of a base (the placeholder is one by construction)."""
    if channel == "input_grad":
        return fused._placeholder_with_input_grad(6, 4, PAYLOAD, None, torch.device("cpu"))
    t = torch.zeros(24).view(6, 4) if view else torch.zeros(6, 4)
    if channel == "zero_colsum":
        fused.mark_zero_colsum(t)
    else:
        fused.mark_maxima(t, PAYLOAD)
    return t


def _accepted(channel, presented):
    if channel == "zero_colsum":
        return fused.has_zero_colsum(presented)
    got = fused.take_maxima(presented) if channel == "maxima" else fused.take_input_grad(presented)
    assert got is None or (got if channel == "maxima" else got[0]) is PAYLOAD
    return got is not None


# what is presented, made from the marked tensor t; every one starts at t's address (the channels are keyed by it)
PRESENTED = {
    "the same object": lambda t: t,
    "a reshape": lambda t: t.view(6, 4) if t.stride(0) == 0 else t.view(2, 3, 4),        # same elements, same last dimension
    "another last dimension": lambda t: t.view(4, 6) if t.stride(0) == 0 else t.view(3, 8),
    "a slice with fewer elements": lambda t: t[:3],
    "a sibling view": lambda t: t._base.as_strided(t.shape, t.stride(), t.storage_offset()),     # of t's base, not of t
}
#                                         zero column sums   maxima   input gradient
RULES = {"the same object":              (True,              True,    True),
         "a reshape":                    (True,              True,    True),
         "another last dimension":       (False,             True,    False),      # the maxima are per row of the same elements
         "a slice with fewer elements":  (False,             False,   False),
         "a sibling view":               (False,             True,    True)}
CASES = [(c, p) for p in RULES for c in CHANNELS]


@pytest.fixture(autouse=True)
def _empty_channels():
    fused.clear_zero_colsum()
    yield
    fused.clear_zero_colsum()


@pytest.mark.parametrize("channel,presented", CASES, ids=["%s: %s" % c for c in CASES])
def test_which_tensor_stands_for_the_marked_one(channel, presented):
    t = _mark(channel, view=presented == "a sibling view")
    p = PRESENTED[presented](t)
    assert p.data_ptr() == t.data_ptr() and (p is t) == (presented == "the same object")
    assert _accepted(channel, p) is RULES[presented][CHANNELS.index(channel)]
    assert not _accepted(channel, t), "taken once: the entry is gone whatever the answer was"


def test_the_input_gradient_is_not_taken_by_a_tensor_with_a_row_stride():
    """take_input_grad looks only at zero-stride tensors: an ordinary gradient at the placeholder's address neither receives the
    carried gradients nor consumes the entry."""
    t = _mark("input_grad")
    assert fused.is_placeholder(t) and not fused.is_placeholder(torch.zeros(6, 4)) and not fused.is_placeholder(t[:1, :1])
    ordinary = t._base.as_strided((2, 2), (2, 1), t.storage_offset())
    assert ordinary.data_ptr() == t.data_ptr() and fused.take_input_grad(ordinary) is None
    assert fused.take_input_grad(t) == (PAYLOAD, None)


@pytest.mark.parametrize("channel", CHANNELS)
def test_a_different_live_tensor_is_refused(channel):
    t = _mark(channel)
    other = torch.full((1,), float("nan")).expand(6, 4) if channel == "input_grad" else torch.zeros(6, 4)
    assert other.data_ptr() != t.data_ptr() and not _accepted(channel, other)
    assert _accepted(channel, t), "another key: the entry is still there"


@pytest.mark.parametrize("channel", CHANNELS)
def test_a_tensor_at_the_address_of_a_dropped_one_is_refused(channel):
    """The key is an address, and addresses are recycled: the weak reference to the marked tensor must still be alive."""
    t = _mark(channel, view=True)
    again = PRESENTED["a sibling view"](t)
    assert again.data_ptr() == t.data_ptr()
    del t
    assert not _accepted(channel, again)


def test_clear_zero_colsum_empties_all_three_channels():
    marked = [_mark(c) for c in CHANNELS]
    fused.clear_zero_colsum()
    assert not any(_accepted(c, t) for c, t in zip(CHANNELS, marked))


def test_route_of_tensors_off_the_device_without_the_library(monkeypatch):
    """Tensors that are not on the device take torch's matmul, with no partials -- decided without asking for the library, which
    a machine without a GPU need not have built."""
    def requested():
        raise AssertionError("the library handle was requested")
    monkeypatch.setattr(fused._lib, "lib", requested)
    x, w = torch.randn(5000, 8), torch.randn(16, 8)
    for bias, addend, want_stats in ((None, None, False), (torch.randn(16), None, True), (None, torch.randn(5000, 16), True)):
        r = fused.dense_route(x, w, bias, addend, None, want_stats)
        assert r.route == "torch" and r.stats is False and r.block_rows == 0 and r.x_maxima is False
    assert fused.stat_block_rows(x, w) == 0
    y, part = fused.linear_cl(x, w, None, None, True)
    assert part is None and torch.equal(y, torch.nn.functional.linear(x, w))
    assert fused.linear_cl(x, w, None, None, False)[1] is None and torch.is_tensor(fused.linear_cl(x, w))
