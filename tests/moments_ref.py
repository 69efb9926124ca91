"""numpy restatement of the weighted moments (include/cusmc_hip.h) and a Kalman filter for
the model the particle filter implements.

Effective weights:
  densities:   M = largest w_i > 0 (NaN excluded); w^_i = w_i / M where w_i > 0, else 0
  log-weights: M = largest non-NaN lw_i; w^_i = exp_nonpos(lw_i - M), NaN and -inf giving 0
With W = sum w^_i:  m = sum w^_i x_i / W;  P = sum w^_i (x_i - m)(x_i - m)^T / W;  ESS = W^2 / sum w^_i^2;
ell = log(W / N) + log M (log-weights: + M).
No positive weight: m, P NaN, ESS 0, ell -inf.  M = +inf: m, P, ESS NaN, ell +inf.
Sums in np.longdouble, two-pass (P about the m of pass 1)."""
import numpy as np

import stratified_ref as R

LD = np.longdouble


def effective(w, log=False):
    """(w^ as float64, M, state) with state "ok", "none" (no positive weight) or "inf" (M = +inf)."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if log:
        ok = ~np.isnan(w)
        if not ok.any():
            return np.zeros_like(w), -np.inf, "none"
        M = float(w[ok].max())
        if M == np.inf:
            return None, M, "inf"
        if M == -np.inf:
            return np.zeros_like(w), M, "none"
        r = np.zeros_like(w)
        fin = ok & (w > -np.inf)
        r[fin] = R.exp_nonpos(w[fin] - M)
        return r, M, "ok"
    pos = w > 0  # (NaN compares false)
    if not pos.any():
        return np.zeros_like(w), 0.0, "none"
    M = float(w[pos].max())
    if M == np.inf:
        return None, M, "inf"
    r = np.zeros_like(w)
    r[pos] = w[pos] / M
    return r, M, "ok"


def moments(X, w, log=False, cov=True):
    """{"mean", "cov", "ess", "loglik_increment"} of the rows of X (N x d) under w, in long double."""
    X = np.asarray(X, dtype=np.float64)
    N, d = X.shape
    wh, M, state = effective(w, log)
    if state == "none":
        return {"mean": np.full(d, np.nan), "cov": np.full((d, d), np.nan) if cov else None, "ess": 0.0,
                "loglik_increment": -np.inf}
    if state == "inf":
        return {"mean": np.full(d, np.nan), "cov": np.full((d, d), np.nan) if cov else None, "ess": np.nan,
                "loglik_increment": np.inf}
    whl = wh.astype(LD)
    Xl = X.astype(LD)
    W = whl.sum()
    m = (whl[:, None] * Xl).sum(0) / W
    out = {"mean": m.astype(np.float64), "ess": float(W * W / (whl * whl).sum()),
           "loglik_increment": float(np.log(W / LD(N)) + (LD(M) if log else np.log(LD(M))))}
    if cov:
        C = Xl - m
        P = (whl[:, None] * C).T @ C / W
        out["cov"] = ((P + P.T) / 2).astype(np.float64)
    else:
        out["cov"] = None
    return out


def error_scales(X, w, log=False):
    """The natural scales of the bounds: sum w^|x_j - m_j| / W, sum w^|x_j - m_j||x_k - m_k| / W, |m|."""
    wh, _, state = effective(w, log)
    X = np.asarray(X, dtype=np.float64).astype(LD)
    whl = wh.astype(LD)
    W = whl.sum()
    m = (whl[:, None] * X).sum(0) / W
    A = np.abs(X - m)
    s1 = (whl[:, None] * A).sum(0) / W
    s2 = (whl[:, None] * A).T @ A / W
    return s1.astype(np.float64), s2.astype(np.float64), np.abs(m).astype(np.float64)


def kalman(Y, m0, C0, F, G, V, W):
    """Filtered means (T x d), covariances (T x d x d) and log-likelihood increments (T; 0 at t = 0) of
    x_0 ~ N(m0, C0), x_t = G x_{t-1} + N(0, W), y_t = F x_t + N(0, V); Y is T x d (row t = y_t; y_0 unused)."""
    Y = np.asarray(Y, dtype=np.float64)
    T, d = Y.shape
    m = np.asarray(m0, dtype=np.float64).reshape(-1).copy()
    P = np.asarray(C0, dtype=np.float64).copy()
    means, covs, ll = [m.copy()], [P.copy()], [0.0]
    for t in range(1, T):
        mp = G @ m
        Pp = G @ P @ G.T + W
        S = F @ Pp @ F.T + V
        r = Y[t] - F @ mp
        Ls = np.linalg.cholesky(S)
        z = np.linalg.solve(Ls, r)
        ll.append(float(-0.5 * z @ z - np.log(np.diag(Ls)).sum() - 0.5 * len(r) * np.log(2 * np.pi)))
        K = np.linalg.solve(S, F @ Pp).T
        m = mp + K @ r
        P = Pp - K @ S @ K.T
        P = (P + P.T) / 2
        means.append(m.copy())
        covs.append(P.copy())
    return np.array(means), np.array(covs), np.array(ll)
