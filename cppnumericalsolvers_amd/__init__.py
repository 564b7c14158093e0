"""cppnumericalsolvers_amd — MI355X-native batched L-BFGS engine.

The hot path of PatWie/CppNumericalSolvers (Solver::Minimize -> Lbfgs ->
MoreThuente -> objective) rebuilt as hand-written HIP for gfx950 behind a C-ABI
(include/mi355_lbfgs.h).  Importing this package does not load the HIP library;
`capi.load()` / `engine.Context()` do, and fail loudly when it is missing.
"""
from . import _build, capi  # noqa: F401
from .engine import (AugLagComposite, BatchedAugmentedLagrangian, BatchedBfgs, BatchedConjugatedGradientDescent, BatchedGradientDescent, BatchedLbfgs, BatchedLbfgsb, BatchedNelderMead, BatchedNewtonDescent, BatchedTrustRegionNewton, ConstrainedProblem, Context, DerivativeCheck, DeviceGroup, DiagQuadratic, LbfgsAskTell, LbfgsbAskTell, Objective, Rosenbrock, Trace,  # noqa: F401
                     SquaredErrorRidge, SquaredErrorRidgePerProblem, ridge_per_problem_rows, al_progress_to_numpy, check_derivatives, parity_stop, progress_to_numpy, synthetic_ridge_host,
                     synthetic_x0_host)

__all__ = ["AugLagComposite", "BatchedAugmentedLagrangian", "ConstrainedProblem", "BatchedBfgs", "BatchedConjugatedGradientDescent", "BatchedGradientDescent", "BatchedLbfgs", "BatchedLbfgsb", "BatchedNelderMead", "BatchedNewtonDescent", "BatchedTrustRegionNewton", "Context", "DeviceGroup", "LbfgsAskTell", "LbfgsbAskTell", "Trace", "DiagQuadratic", "Objective", "Rosenbrock", "SquaredErrorRidge", "SquaredErrorRidgePerProblem", "ridge_per_problem_rows", "parity_stop",
           "al_progress_to_numpy", "check_derivatives", "DerivativeCheck", "progress_to_numpy", "synthetic_ridge_host", "synthetic_x0_host", "capi"]
