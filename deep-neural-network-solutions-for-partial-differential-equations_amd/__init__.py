"""MI355X-native deep-BSDE (FBSNN) training step.

The hot path -- Euler-Maruyama rollout, NAIS-Net/FC subnetwork forward with
Z = grad_x u, residual loss, second-order backward, clip + Adam -- runs as
hand-written HIP kernels for gfx950 behind the C ABI of include/dbsde.h
(lib/libdbsde.so).  This package is the host side: the reference's FBSNN
class surface (nd_BSPDE_case.py / DeepBSDE.py) over that ABI.

Import it with importlib (the directory name is not a Python identifier):
    pkg = importlib.import_module(
        "deep-neural-network-solutions-for-partial-differential-equations_amd")
"""
from . import _lib
from .deepbsde import BlackScholesBarenblatt, u_exact
from .fbsnn import FBSNN, PredictionGenerator
from .problems import (AmericanBasketPutOption, AmericanPutOption, BarrierBasketCallOption, BarrierBasketPutOption,
                       BarrierCallOption, BarrierPutOption, AsianBasketCallOption, AsianBasketPutOption, AsianCallOption, AsianPutOption,
                       BasketCallOption, BasketPutOption, BSPDETestCase, CallOption, CallOption1D,
                       GeometricAsianBasketCallOption, GeometricAsianBasketPutOption, GeometricAsianCallOption,
                       GeometricAsianPutOption, HamiltonJacobiBellman, HestonFBSNN, HestonTwoFactorFBSNN, PutOption)
from .solver import NativeSolver, ProblemSpec, exact, free_call_profile, hjb_mc, mc_value

__all__ = ["FBSNN", "PredictionGenerator", "BlackScholesBarenblatt", "u_exact", "CallOption", "PutOption",
           "CallOption1D", "BasketCallOption", "BasketPutOption", "BSPDETestCase", "HamiltonJacobiBellman",
           "HestonFBSNN", "HestonTwoFactorFBSNN",
           "AsianCallOption", "AsianPutOption", "AsianBasketCallOption", "AsianBasketPutOption",
           "GeometricAsianCallOption", "GeometricAsianPutOption", "GeometricAsianBasketCallOption",
           "GeometricAsianBasketPutOption", "AmericanPutOption", "AmericanBasketPutOption",
           "BarrierCallOption", "BarrierPutOption", "BarrierBasketCallOption", "BarrierBasketPutOption",
           "NativeSolver", "ProblemSpec", "exact", "free_call_profile", "hjb_mc", "mc_value", "_lib"]
