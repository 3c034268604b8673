"""Drop-in for the reference's ``evaluation/StructuralLosses`` package
(``match_cost``, ``nn_distance``) on libpdgn_hip.so, and the exact EMD of equal-sized clouds
(``exact_emd_cost``, ``auction_match``: no reference counterpart)."""
from .exact_emd import ExactEMDFunction, auction_match, exact_emd_cost  # noqa: F401
from .match_cost import match_cost, emd_cost  # noqa: F401
from .nn_distance import nn_distance  # noqa: F401
