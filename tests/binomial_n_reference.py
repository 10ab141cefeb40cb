"""Float64 restatement of the binomial likelihood with per-point trial counts (AGPL_LIK_BINOMIAL_N = 11, include/agpl.h): every
rule is tests/binomial_reference.py's, called with the trials of the point at hand -- points are grouped by their n and each
group goes through that file's functions, so nothing of its arithmetic (the Polya-Gamma mean, the mass function's integration)
is restated here."""
import numpy as np

import binomial_reference as B

KIND = 11


def by_trials(trials):
    """(n, index array) for every distinct trial count."""
    trials = np.asarray(trials)
    return [(int(n), np.nonzero(trials == n)[0]) for n in np.unique(trials)]


def expected_potential_precision(trials, y, c):
    beta, gamma = np.empty(len(y)), np.empty(len(y))
    for n, idx in by_trials(trials):
        beta[idx], gamma[idx] = B.expected_potential_precision(n, y[idx], c[idx])
    return beta, gamma


def sampled_potential_precision(trials, y, omega):
    beta = np.empty(len(y))
    for n, idx in by_trials(trials):
        beta[idx] = B.sampled_potential_precision(n, y[idx], omega[idx])[0]
    return beta, omega


def elbo_terms(trials, y, mu, var):
    return sum(B.elbo_terms(n, y[idx], mu[idx], var[idx]) for n, idx in by_trials(trials))


def pmf(n, mu, s):
    """p(y), y = 0 .. n, of one point: binomial_reference's mass function at that point's n."""
    return B.pmf_all(int(n), float(mu), float(s))


def moments(n, mu, var):
    return B.ref_moments(int(n), float(mu), float(var))


def cavi_sweeps(trials, Phi, kdiag, y, nsweeps):
    """binomial_reference.cavi_sweeps with the trials of each point: the same loop, its per-point rules called per group of n."""
    N, M = Phi.shape
    S, m = np.eye(M), np.zeros(M)
    y = y.astype(np.float64)
    out = dict(G=[], g=[], S=[], m=[], elbo=[])
    for _ in range(nsweeps):
        mu = Phi @ m
        var = kdiag + np.einsum("ia,ab,ib->i", Phi, S, Phi)
        beta, gamma = expected_potential_precision(trials, y, B.aux_posterior(mu, var))
        klv = 0.5 * (np.trace(S) + m @ m - M - np.linalg.slogdet(S)[1])
        out["elbo"].append(elbo_terms(trials, y, mu, var) - klv)
        G = (Phi * gamma[:, None]).T @ Phi
        g = Phi.T @ beta
        S = np.linalg.inv(np.eye(M) + G)
        S = 0.5 * (S + S.T)
        m = S @ g
        for k, v in (("G", G), ("g", g), ("S", S), ("m", m)):
            out[k].append(v)
    return out


def expand(trials, y, *rows):
    """The same data as sum(trials) Bernoulli rows: point i becomes n_i rows, y_i of them ones; every array of ``rows`` is
    replicated alongside.  Returns (y01 uint8, replicated rows...)."""
    trials, y = np.asarray(trials), np.asarray(y)
    rep = np.repeat(np.arange(len(y)), trials)
    first = np.cumsum(trials) - trials
    y01 = (np.arange(len(rep)) - first[rep] < y[rep]).astype(np.uint8)
    return (y01,) + tuple(np.asarray(r)[rep] for r in rows)
