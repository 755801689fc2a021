"""MI355X-native posterior / logpdf / marginals / rand path of BayesianLinearRegressors.jl.

Import as ``import blr_amd`` (the directory name follows the reference repository and is not a valid
Python identifier; ``blr_amd.py`` at the repository root loads it under that name).

Exports mirror reference src/BayesianLinearRegressors.jl:11-12.
"""
from . import _abi
from ._abi import BLRError, PosDefException
from .regressor import (
    BasisFunctionRegressor,
    BayesianLinearRegressor,
    BLRFunctionSample,
    ColVecs,
    Diagonal,
    EvidenceGrid,
    FiniteGP,
    LOO,
    Normal,
    PDMat,
    RandomFourierFeatures,
    ResidentPosterior,
    ResidentColumnsPosterior,
    RowVecs,
    Symmetric,
    cov,
    evaluate,
    logpdf,
    logpdf_and_gradient,
    logpdf_columns,
    logpdf_columns_map,
    logpdf_grid,
    logpdf_grid_map,
    logpdf_map,
    logpdf_ragged,
    loo,
    loo_columns,
    loo_columns_map,
    loo_map,
    marginals,
    mean,
    mean_and_cov,
    mean_and_var,
    mean_and_var_columns,
    mean_and_var_columns_map,
    cov_map,
    mean_and_cov_map,
    mean_columns,
    posterior,
    posterior_best,
    posterior_columns,
    posterior_columns_map,
    posterior_map,
    posterior_ragged,
    rand,
    rand_and_pullback,
    rand_b,
    rand_map,
    std,
    var,
)

__all__ = [
    "logpdf", "rand", "mean", "std", "cov", "var", "BayesianLinearRegressor", "marginals", "posterior",
    "BasisFunctionRegressor", "ColVecs", "RowVecs", "Diagonal", "Symmetric", "PDMat", "Normal", "FiniteGP",
    "BLRFunctionSample", "RandomFourierFeatures", "mean_and_var", "mean_and_cov", "rand_b", "rand_and_pullback", "evaluate", "logpdf_columns", "logpdf_and_gradient", "logpdf_map", "posterior_map", "rand_map", "BLRError", "PosDefException", "ResidentPosterior", "ResidentColumnsPosterior",
    "LOO", "loo", "loo_map", "loo_columns", "loo_columns_map",
    "EvidenceGrid", "logpdf_grid", "posterior_best", "logpdf_grid_map",
    "posterior_ragged", "logpdf_ragged",
    "posterior_columns", "logpdf_columns_map", "posterior_columns_map",
    "mean_and_var_columns", "mean_columns", "mean_and_var_columns_map",
    "cov_map", "mean_and_cov_map",
]
