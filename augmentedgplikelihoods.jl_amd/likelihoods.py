"""Likelihood types = constructor arguments of the reference's likelihoods (src/likelihoods/*.jl and the
re-exported GPLikelihoods types).  They only carry parameters; all arithmetic is in libagpl.so."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from ._ffi import LikDesc

(KIND_BERNOULLI, KIND_NEGBINOMIAL, KIND_STUDENTT, KIND_CATEGORICAL, KIND_CATEGORICAL_BIJ, KIND_POISSON,
 KIND_LAPLACE, KIND_HETEROGAUSS, KIND_BINOMIAL, KIND_ASYMLAPLACE, KIND_LOGISTIC_NOISE, KIND_BINOMIAL_N) = range(12)


class AbstractLikelihood:
    kind: int = -1
    _nlatent: int = 1

    def _params(self):
        return ()

    def _logtheta(self):
        return None

    # the fields behind the descriptor's p[], in its order: the parameters whose logarithms agpl_expected_loglik differentiates
    _param_names = ()

    def desc(self) -> LikDesc:
        d = LikDesc()
        d.kind, d.nlatent = self.kind, self._nlatent
        p = list(self._params()) + [0.0] * 4
        for i in range(4):
            d.p[i] = float(p[i])
        lt = self._logtheta()
        if lt is not None:
            self._lt_keep = np.ascontiguousarray(lt, dtype=np.float64)
            d.logtheta = self._lt_keep.ctypes.data_as(C.POINTER(C.c_double))
        return d

    # dtype of y on the device: 'u8' | 'i32' | 'real' | 'i32x2' (int32 [N, 2], point-major: successes, trials)
    ykind = "real"


def nlatent(lik: AbstractLikelihood) -> int:
    """nlatent(lik): src/generic.jl:87, src/likelihoods/categorical.jl:46-47,
    src/likelihoods/heteroscedasticgaussian.jl:11."""
    return lik._nlatent


@dataclass
class BernoulliLikelihood(AbstractLikelihood):
    """BernoulliLikelihood(LogisticLink()) -- src/likelihoods/bernoulli.jl."""
    kind = KIND_BERNOULLI
    ykind = "u8"


@dataclass
class NegativeBinomialLikelihood(AbstractLikelihood):
    """NegativeBinomialLikelihood(NBParamFailure(r), LogisticLink()) -- src/likelihoods/negativebinomial.jl."""
    failures: float = 1.0
    kind = KIND_NEGBINOMIAL
    ykind = "i32"
    _param_names = ("failures",)

    def _params(self):
        return (self.failures,)


@dataclass
class StudentTLikelihood(AbstractLikelihood):
    """StudentTLikelihood(nu, sigma) -- src/likelihoods/studentt.jl:14-21."""
    nu: float = 3.0
    sigma: float = 1.0
    kind = KIND_STUDENTT
    _param_names = ("nu", "sigma")

    def _params(self):
        return (self.nu, self.sigma)


@dataclass
class CategoricalLikelihood(AbstractLikelihood):
    """CategoricalLikelihood(LogisticSoftMaxLink(logtheta)) or, with ``bijective=True``,
    CategoricalLikelihood(BijectiveSimplexLink(LogisticSoftMaxLink(logtheta))) --
    src/likelihoods/categorical.jl:6-47.  ``CategoricalLikelihood(nclass)`` = zeros(nclass) (:10)."""
    logtheta: object = 2
    bijective: bool = False
    ykind = "u8"

    def __post_init__(self):
        if isinstance(self.logtheta, (int, np.integer)):
            self.logtheta = np.zeros(int(self.logtheta))
        self.logtheta = np.asarray(self.logtheta, dtype=np.float64)
        self.kind = KIND_CATEGORICAL_BIJ if self.bijective else KIND_CATEGORICAL
        self._nlatent = len(self.logtheta) - (1 if self.bijective else 0)

    def _logtheta(self):
        return self.logtheta


@dataclass
class PoissonLikelihood(AbstractLikelihood):
    """PoissonLikelihood(ScaledLogistic(lambda)) -- src/likelihoods/poisson.jl."""
    lam: float = 1.0
    kind = KIND_POISSON
    ykind = "i32"
    _param_names = ("lam",)

    def _params(self):
        return (self.lam,)


@dataclass
class LaplaceLikelihood(AbstractLikelihood):
    """LaplaceLikelihood(beta) -- src/likelihoods/laplace.jl:13-17."""
    beta: float = 1.0
    kind = KIND_LAPLACE
    _param_names = ("beta",)

    def _params(self):
        return (self.beta,)


@dataclass
class HeteroscedasticGaussianLikelihood(AbstractLikelihood):
    """HeteroscedasticGaussianLikelihood(InvScaledLogistic(lambda)) --
    src/likelihoods/heteroscedasticgaussian.jl."""
    lam: float = 1.0
    kind = KIND_HETEROGAUSS
    _nlatent = 2
    _param_names = ("lam",)

    def _params(self):
        return (self.lam,)


@dataclass
class BinomialLikelihood(AbstractLikelihood):
    """Binomial(n, logistic(f)): y successes out of ``n`` trials, the same n at every point (an integer, 1 <= n < 2^22).  No
    file in the reference: the Polya-Gamma identity behind its Bernoulli and negative-binomial augmentations holds for any
    exponent pair (include/agpl.h, AGPL_LIK_BINOMIAL).  ``n`` is data, not a learnable parameter."""
    n: int = 1
    kind = KIND_BINOMIAL
    ykind = "i32"

    def _params(self):
        return (self.n,)


@dataclass
class AsymmetricLaplaceLikelihood(AbstractLikelihood):
    """Asymmetric Laplace likelihood: the negative log density is the pinball loss of (y - f) / sigma at level ``tau``, so the
    latent f(x) is the tau-quantile of y | x (quantile regression).  No file in the reference: an exponential tilt of its
    Laplace likelihood at beta = 2 sigma (include/agpl.h, AGPL_LIK_ASYMLAPLACE).  ``sigma`` is the one learnable parameter;
    ``tau`` (0 < tau < 1) is the chosen level, not a parameter."""
    tau: float = 0.5
    sigma: float = 1.0
    kind = KIND_ASYMLAPLACE
    _param_names = ("sigma",)

    def _params(self):
        return (self.sigma, self.tau)


@dataclass
class LogisticNoiseLikelihood(AbstractLikelihood):
    """Logistic noise, y = f + scale * eps with eps ~ Logistic(0, 1): the likelihood whose negative log density is the log-cosh
    loss, 2 logcosh((y - f) / (2 scale)) + log(4 scale) -- Gaussian-like around the residual's origin, exponential tails beyond.
    No file in the reference: its Polya-Gamma identity at the exponent pair (1, 1), applied to the residual (include/agpl.h,
    AGPL_LIK_LOGISTIC_NOISE).  ``scale`` is the one learnable parameter."""
    scale: float = 1.0
    kind = KIND_LOGISTIC_NOISE
    _param_names = ("scale",)

    def _params(self):
        return (self.scale,)


@dataclass
class BinomialTrialsLikelihood(AbstractLikelihood):
    """Binomial(n_i, logistic(f_i)) with a trial count of its own at every point: ``BinomialLikelihood`` with n read from the
    observation.  ``y`` is int32 ``[N, 2]`` -- column 0 the successes, column 1 the trials, 1 <= n_i < 2^22 (``binomial_obs``
    builds and checks it).  No parameters (include/agpl.h, AGPL_LIK_BINOMIAL_N)."""
    kind = KIND_BINOMIAL_N
    ykind = "i32x2"


def binomial_obs(y, trials):
    """The observation of ``BinomialTrialsLikelihood``: int32 ``[N, 2]`` with column 0 = ``y`` (successes, 0 <= y) and column 1 =
    ``trials`` (1 <= trials < 2^22), on the device the inputs are on.  Raises ArgumentError naming the first offending index."""
    import torch

    from ._ffi import ERR_INVALID_ARGUMENT, ArgumentError

    y, trials = torch.as_tensor(y), torch.as_tensor(trials)
    if y.ndim != 1 or trials.ndim != 1 or y.shape[0] != trials.shape[0]:
        raise ArgumentError(ERR_INVALID_ARGUMENT, f"binomial_obs: y and trials must be vectors of one length (got {tuple(y.shape)} and {tuple(trials.shape)})")
    trials = trials.to(y.device)
    for name, bad in (("y", (y < 0) | (y != torch.floor(y))), ("trials", ~((trials >= 1) & (trials < 4194304)) | (trials != torch.floor(trials)))):
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            val = (y if name == "y" else trials)[i].item()
            want = "an integer >= 0" if name == "y" else "an integer with 1 <= trials < 4194304 = 2^22"
            raise ArgumentError(ERR_INVALID_ARGUMENT, f"binomial_obs: {name}[{i}] = {val} must be {want}")
    return torch.stack([y.to(torch.int32), trials.to(torch.int32)], dim=1).contiguous()
