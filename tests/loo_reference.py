"""numpy float64 reference of the leave-one-out cavity (include/agpl_loo.h).  Three routes to the same numbers:

  * ``closed_form``   Sherman-Morrison on the marginals of q(v): var_-i = d + q / (1 - h), mu_-i = mu0 + (a - beta q) / (1 - h);
  * ``refit``         brute force: for every (latent, point) invert I + G - gamma_i phi_i phi_i' and solve for the mean;
  * ``rule``          the header's rule restated on the host, from float32 inputs, operation by operation in the header's order --
                      what the device kernel must reproduce bit for bit.

Layouts: Phi [N, M]; gamma, beta, mu0 [L, N]; d [N]; eta0 [L, M] or None.  ``closed_form`` and ``refit`` return (mu, var, h) [L, N];
``rule`` returns the device's point-major (mu, var, h) [N, L], the leverage sums' operands, the count and the lowest flat index."""
import numpy as np

f64, f32 = np.float64, np.float32


def posterior(Phi, gamma, beta, eta0=None):
    """(S, m, G, g) of q(v) as agpl_plan_update forms it: G = Phi' diag(gamma) Phi, g = Phi' beta, S = (I + G)^-1, m = S (g + eta0)."""
    P = Phi.astype(f64)
    L, M = gamma.shape[0], P.shape[1]
    G = np.stack([(P.T * gamma[l].astype(f64)[None]) @ P for l in range(L)])
    g = beta.astype(f64) @ P
    e0 = np.zeros((L, M)) if eta0 is None else eta0.astype(f64)
    S = np.linalg.inv(np.eye(M)[None] + G)
    m = np.einsum("lab,lb->la", S, g + e0)
    return S, m, G, g


def marginals(Phi, d, S, m, mu0=None):
    """(mu, var) [L, N] of f_i under q(v): mu = mu0 + phi'm, var = d + phi'S phi."""
    P = Phi.astype(f64)
    q = np.stack([((P @ S[l]) * P).sum(1) for l in range(S.shape[0])])
    a = m @ P.T
    m0 = 0.0 if mu0 is None else mu0.astype(f64)
    return m0 + a, d.astype(f64)[None] + q


def closed_form(Phi, d, gamma, beta, mu0=None, eta0=None, post=None):
    """``post``: the result of ``posterior`` for these arguments, if the caller has it."""
    P = Phi.astype(f64)
    S, m, _, _ = post or posterior(Phi, gamma, beta, eta0)
    q = np.stack([((P @ S[l]) * P).sum(1) for l in range(S.shape[0])])
    a = m @ P.T
    h = gamma.astype(f64) * q
    m0 = 0.0 if mu0 is None else mu0.astype(f64)
    return m0 + (a - beta.astype(f64) * q) / (1.0 - h), d.astype(f64)[None] + q / (1.0 - h), h


def refit(Phi, d, gamma, beta, mu0=None, eta0=None, points=None, post=None):
    """The cavity by brute force: one M x M inverse per (latent, point).  ``points``: the point indices to refit (all by default);
    the result is [L, len(points)]."""
    P = Phi.astype(f64)
    N, M = P.shape
    L = gamma.shape[0]
    points = np.arange(N) if points is None else np.asarray(points)
    _, _, G, g = post or posterior(Phi, gamma, beta, eta0)
    e0 = np.zeros((L, M)) if eta0 is None else eta0.astype(f64)
    mu, var = np.zeros((L, points.size)), np.zeros((L, points.size))
    for l in range(L):
        A = np.eye(M) + G[l]
        r = g[l] + e0[l]
        for k, i in enumerate(points):
            ph = P[i]
            Si = np.linalg.inv(A - f64(gamma[l, i]) * np.outer(ph, ph))
            mi = Si @ (r - f64(beta[l, i]) * ph)
            var[l, k] = f64(d[i]) + ph @ Si @ ph
            mu[l, k] = ph @ mi
    if mu0 is not None:
        mu = mu + mu0.astype(f64)[:, points]
    return mu, var


def rule(mu, var, d, gamma, beta, mu0=None):
    """THE RULE of include/agpl_loo.h on the host.  mu, var, gamma, beta, mu0 float32 [L, N], d float32 [N].  Every line below is one
    IEEE float64 operation on arrays, in the header's order; numpy fuses nothing.  Returns a dict: mu, var, lev float64 [N, L]
    (NaN where there is no cavity), h_in [L, N] (the leverages as they enter lev_sum: 0 where there is no cavity), n_bad, first_bad."""
    for t in (mu, var, d, gamma, beta) + (() if mu0 is None else (mu0,)):
        assert t.dtype == f32
    L, N = mu.shape
    with np.errstate(all="ignore"):
        muf, varf, g, b = (t.astype(f64) for t in (mu, var, gamma, beta))
        dd = np.broadcast_to(d.astype(f64)[None], (L, N))
        m0 = np.zeros((L, N)) if mu0 is None else mu0.astype(f64)
        ok = np.isfinite(mu) & np.isfinite(var) & np.isfinite(gamma) & np.isfinite(beta) & ~(gamma < 0)
        q = varf - dd
        q = np.where(q > 0, q, 0.0)
        a = muf - m0
        h = g * q
        ok = ok & (h < 1.0)
        t = 1.0 - h
        vo = dd + q / t
        u = b * q
        w = a - u
        mo = m0 + w / t
    nan = np.full((L, N), np.nan)
    bad = np.flatnonzero(~ok.reshape(-1))
    return {"mu": np.ascontiguousarray(np.where(ok, mo, nan).T), "var": np.ascontiguousarray(np.where(ok, vo, nan).T),
            "lev": np.ascontiguousarray(np.where(ok, h, nan).T), "h_in": np.where(ok, h, 0.0), "n_bad": int(bad.size),
            "first_bad": int(bad[0]) if bad.size else -1}


def lev_sum(h_in, threads=256, partials=1024):
    """lev_sum in the header's order, from the leverages as they enter it (``rule``'s h_in [L, N])."""
    L, N = h_in.shape
    tiles = -(-N // threads)
    B = min(tiles, partials)
    out = np.zeros(L)
    for l in range(L):
        hp = np.zeros(tiles * threads)
        hp[:N] = h_in[l]
        s = hp.reshape(tiles, threads // 64, 64).copy()  # [tile, wave, lane]
        o = 32
        while o:  # the butterfly: lane k adds lane k ^ o; every lane ends with the same sum
            s = s + s[..., np.arange(64) ^ o]
            o >>= 1
        wsum = s[..., 0]  # [tile, wave]
        part = np.zeros(B)
        for b in range(B):
            acc = np.zeros(threads // 64)
            for t in range(b, tiles, B):
                acc = acc + wsum[t]
            p = acc[0]
            for w in range(1, threads // 64):
                p = p + acc[w]
            part[b] = p
        red = np.zeros(threads)
        for j in range(min(threads, B)):
            t = 0.0
            for k in range(j, B, threads):
                t = t + part[k]
            red[j] = t
        st = threads // 2
        while st:
            red[:st] = red[:st] + red[st:2 * st]
            st //= 2
        out[l] = red[0]
    return out


def case(N=300, M=40, L=2, seed=7, high=0.99, with_mu0=True, with_eta0=True):
    """Random float32 features with free sites: point 0 is isolated (its own feature column) and its gamma is set so that its leverage
    is ``high`` in latent 0; point 1 has gamma = 0 in every latent.  Returns a dict of float32 / float64 arrays."""
    rng = np.random.default_rng(seed)
    Phi = (rng.standard_normal((N, M)) * 0.2).astype(f32)
    d = (rng.random(N) * 0.5).astype(f32)
    gamma = (rng.random((L, N)) * 0.8).astype(f32)
    beta = rng.standard_normal((L, N)).astype(f32)
    if N > 1 and high is not None:
        # isolate point 0: feature column 0 belongs to it alone.  Then q_0 = s / (1 + gamma s) with s = phi_00^2 + (a small rest), and
        # h_0 = gamma s / (1 + gamma s) = high at gamma = high / ((1 - high) s)
        Phi[:, 0] = 0
        Phi[0, :] = 0
        Phi[0, 0] = 1.5
        gamma[0, 0] = f32(high / ((1.0 - high) * 1.5 ** 2))
    if N > 1:
        gamma[:, 1] = 0
    mu0 = rng.standard_normal((L, N)).astype(f32) if with_mu0 else None
    eta0 = rng.standard_normal((L, M)) * 0.3 if with_eta0 else None
    return {"Phi": Phi, "d": d, "gamma": gamma, "beta": beta, "mu0": mu0, "eta0": eta0}
