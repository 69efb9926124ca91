"""Weighted moments and filter summaries (include/cusmc_hip.h): the restatement's own laws
and the ABI surface on the CPU; on an MI355X (-m gpu) the kernels against the long-double restatement, bitwise
determinism, the filter's summaries against the standalone call, the history-free filter, and the summaries'
statistics against an exact Kalman filter."""
import ctypes as C
import math
import os
import subprocess
import textwrap

import numpy as np
import pytest

from conftest import ROOT
import moments_ref as MR

NAMES = ["cusmc_moments_dev", "cusmc_moments_log_dev", "cusmc_moments_host", "cusmc_moments_log_host",
         "cusmc_pf_run_summary_host"]
U = 2.0 ** -53
# The bound constant, fixed before any GPU run.  The kernels' sequential chains ("Summation
# depth") are ceil(chunk / 256) rows per pass-1 lane, 16 wave sums in the combine, chunk / 4 MFMA k-steps per
# accumulator and ceil(nchunks / 64) run sums per covariance-reduce slice; at the sizes compared against the
# long-double reference below (N <= 1e5 at d <= 17, N <= 6000 above) none is longer than 32, so C = 64 covers
# them.  At larger N the chains grow with the chunk size and C = 64 is not a proven bound there.
CB = 64


def _families(rng, N):
    """weight families: (name, weights, log form?) -- those of test_stratified_resampler.py, plus a dominant
    particle far from the others and weights near 1e+-300"""
    x = rng.standard_normal((N, 2))
    dens = np.exp(-0.5 * (x ** 2).sum(1) / 0.3) / (2 * np.pi * 0.3)
    zeros = dens.copy()
    zeros[rng.random(N) < 0.5] = 0.0
    neg = dens.copy()
    neg[rng.random(N) < 0.3] *= -1.0
    nan = dens.copy()
    nan[rng.random(N) < 0.2] = np.nan
    dominant = np.full(N, 1e-12)
    dominant[rng.integers(N)] = 1.0
    lw = np.log(dens)
    lw_inf = lw.copy()
    lw_inf[rng.random(N) < 0.4] = -np.inf
    lw_nan = lw - 800.0
    lw_nan[rng.random(N) < 0.1] = np.nan
    return [("dens", dens, False), ("zeros", zeros, False), ("neg", neg, False), ("nan", nan, False),
            ("equal", np.full(N, 0.25), False), ("dominant", dominant, False),
            ("all_zero", np.zeros(N), False), ("pinf", np.where(np.arange(N) == N // 2, np.inf, dens), False),
            ("all_nan", np.full(N, np.nan), False),
            ("log", lw, True), ("log_minf", lw_inf, True), ("log_nan", lw_nan, True),
            ("log_all_minf", np.full(N, -np.inf), True), ("log_pinf", np.where(np.arange(N) == 0, np.inf, lw), True),
            ("huge", dens * 1e300, False), ("tiny", dens * 1e-300, False)]


def _points(rng, N, d, far=None):
    X = rng.standard_normal((N, d)) * (1.0 + np.arange(d) / 4.0) + np.arange(d)
    if far is not None:
        X[far] += 1e6  # the dominant particle far from its chunk's others
    return X


# --- the restatement (CPU) ------------------------------------------------------------------------------------

def test_scaling_the_weights_shifts_only_ell():
    rng = np.random.default_rng(0)
    X = _points(rng, 500, 3)
    w = rng.random(500)
    a = MR.moments(X, w)
    for c in (1e-200, 0.5, 3.0, 1e200):
        b = MR.moments(X, w * c)
        assert np.allclose(b["mean"], a["mean"], rtol=1e-14, atol=1e-14)
        assert np.allclose(b["cov"], a["cov"], rtol=1e-13, atol=1e-14)
        assert abs(b["ess"] - a["ess"]) <= 1e-12 * a["ess"]
        assert abs(b["loglik_increment"] - (a["loglik_increment"] + math.log(c))) <= 1e-12 * (1 + abs(math.log(c)))


def test_log_form_equals_density_form():
    rng = np.random.default_rng(1)
    X = _points(rng, 400, 4)
    w = rng.random(400) + 0.01
    a, b = MR.moments(X, w), MR.moments(X, np.log(w), log=True)
    assert np.allclose(a["mean"], b["mean"], rtol=1e-13)
    assert np.allclose(a["cov"], b["cov"], rtol=1e-12)
    assert abs(a["ess"] - b["ess"]) <= 1e-12 * a["ess"]
    assert abs(a["loglik_increment"] - b["loglik_increment"]) <= 1e-12


def test_degenerate_rules():
    X = np.arange(6.0).reshape(3, 2)
    for w, log in (([0.0, 0.0, 0.0], False), ([-1.0, np.nan, 0.0], False), ([-np.inf, np.nan, -np.inf], True)):
        r = MR.moments(X, np.array(w), log=log)
        assert np.isnan(r["mean"]).all() and np.isnan(r["cov"]).all()
        assert r["ess"] == 0.0 and r["loglik_increment"] == -np.inf
    for w, log in (([1.0, np.inf, 0.0], False), ([0.0, np.inf, np.nan], True)):
        r = MR.moments(X, np.array(w), log=log)
        assert np.isnan(r["mean"]).all() and np.isnan(r["cov"]).all() and np.isnan(r["ess"])
        assert r["loglik_increment"] == np.inf
    # zero, negative and NaN weights count as 0
    r = MR.moments(X, np.array([1.0, np.nan, -2.0]))
    assert np.array_equal(r["mean"], X[0]) and np.array_equal(r["cov"], np.zeros((2, 2)))
    assert r["ess"] == 1.0 and r["loglik_increment"] == pytest.approx(math.log(1.0 / 3.0))


def test_equal_weights_give_sample_moments():
    rng = np.random.default_rng(2)
    X = _points(rng, 300, 3)
    r = MR.moments(X, np.full(300, 1.0 / 300))
    assert np.allclose(r["mean"], X.mean(0), rtol=1e-14)
    assert np.allclose(r["cov"], np.cov(X.T, bias=True), rtol=1e-12)
    assert r["ess"] == pytest.approx(300.0, rel=1e-14)
    assert r["loglik_increment"] == pytest.approx(-math.log(300.0), rel=1e-14)


def test_kalman_matches_the_scalar_closed_form():
    g, q, r, m0, c0 = 0.8, 0.3, 0.5, 0.2, 1.5
    Y = np.array([[9.0], [1.0], [-0.5], [0.7]])
    M, P, L = MR.kalman(Y, [m0], [[c0]], np.eye(1), np.array([[g]]), np.array([[r]]), np.array([[q]]))
    m, p = m0, c0
    assert M[0, 0] == m0 and P[0, 0, 0] == c0 and L[0] == 0.0
    for t in range(1, 4):
        mp, pp = g * m, g * g * p + q
        s = pp + r
        ll = -0.5 * math.log(2 * math.pi * s) - 0.5 * (Y[t, 0] - mp) ** 2 / s
        k = pp / s
        m, p = mp + k * (Y[t, 0] - mp), (1 - k) * pp
        assert M[t, 0] == pytest.approx(m, rel=1e-14) and P[t, 0, 0] == pytest.approx(p, rel=1e-14)
        assert L[t] == pytest.approx(ll, rel=1e-14)


# --- the ABI without a device ---------------------------------------------------------------------------------

def test_header_and_library_carry_the_new_symbols():
    import re
    from cusmc_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cusmc_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name) and name in bound, name


def test_argument_errors_without_a_device():
    from cusmc_amd import _lib
    L = _lib.lib()
    x = (C.c_double * 64)()
    w = (C.c_double * 8)()
    out = (C.c_double * 64)()
    st = (C.c_double * 2)()
    for host in (L.cusmc_moments_host, L.cusmc_moments_log_host, L.cusmc_moments_dev, L.cusmc_moments_log_dev):
        assert host(None, x, 0, 2, 2, w, out, None, st) == _lib.EINVAL      # N = 0
        assert host(None, x, 4, 1, 2, w, out, None, st) == _lib.EINVAL      # ldx < d
        assert host(None, x, 4, 2, 0, w, out, None, st) == _lib.EINVAL      # d < 1
        assert host(None, None, 4, 2, 2, w, out, None, st) == _lib.EINVAL   # null X
        assert host(None, x, 4, 2, 2, None, out, None, st) == _lib.EINVAL   # null w
        assert host(None, x, 4, 2, 2, w, None, None, st) == _lib.EINVAL     # null mean
        assert host(None, x, 4, 2, 2, w, out, None, None) == _lib.EINVAL    # null stats
        assert host(None, x, 4, 400, 385, w, out, None, st) == _lib.ERANGE  # d > CUSMC_MAX_DIM
        assert b"CUSMC_MAX_DIM" in L.cusmc_last_error()


def _summary_call(ctx, T=3, d=2, N=8, summaries=True):
    from cusmc_amd import _lib
    I = np.eye(d).ravel()
    Y = np.zeros(T * d)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mean, ess = np.empty(T * d), np.empty(T)
    return _lib.lib().cusmc_pf_run_summary_host(ctx, p(Y), N, d, T, p(np.zeros(d)), p(I), p(I), p(I), p(I), p(I),
                                                C.c_float(0), b"stratified", b"mvn", 10, 1.0, 1, None, None, None,
                                                p(mean) if summaries else None, None, p(ess) if summaries else None,
                                                None)


def test_sharded_filter_refuses_summaries(monkeypatch):
    """CUSMC_DEVICES set: any summary output is CUSMC_EINVAL before any work (no context is even needed)."""
    from cusmc_amd import _lib
    monkeypatch.setenv("CUSMC_DEVICES", "0,0")
    assert _summary_call(None) == _lib.EINVAL
    assert b"sharded" in _lib.lib().cusmc_last_error()


def test_python_wrappers_validate_before_the_abi():
    import torch
    import cusmc_amd
    from cusmc_amd import api
    with pytest.raises(ValueError):
        cusmc_amd.weighted_moments(np.zeros((4, 2)), np.ones(3), ctx=object())
    with pytest.raises(ValueError):
        cusmc_amd.weighted_moments(np.zeros((0, 2)), np.ones(0), ctx=object())
    x = torch.zeros(8, 4, dtype=torch.float64)
    v = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError):  # CPU tensors
        api.weighted_moments_dev(x, torch.zeros(8, dtype=torch.float64), v, None, torch.zeros(2, dtype=torch.float64),
                                 ctx=object())
    # a broadcast view (row stride 0) and overlapping rows are refused before any pointer is taken
    for bad in (torch.zeros(1, 4, dtype=torch.float64).expand(8, 4),
                torch.zeros(20, dtype=torch.float64).as_strided((8, 4), (2, 1))):
        with pytest.raises(ValueError, match="overlap"):
            api.weighted_moments_dev(bad, torch.zeros(8, dtype=torch.float64), v, None,
                                     torch.zeros(2, dtype=torch.float64), ctx=object())
    I = np.eye(2)
    args = (8, 2, 3, np.zeros((2, 3)), np.zeros(2), I, I, I, I, I, 0.0, "stratified", "mvn")
    for kw in ({"history": False}, {"history": False, "summaries": True, "write_csv": True},
               {"history": False, "summaries": True, "return_ancestors": True},
               {"summaries": True, "devices": [0, 0]}):
        with pytest.raises(ValueError):
            cusmc_amd.run(*args, seed=1, **kw)


# --- on the GPU -----------------------------------------------------------------------------------------------

def _host(X, N, ldx, d, w, log, cov=True, ctx=None):
    """cusmc_moments_host on the first N rows of X (ldx doubles apart, d components)."""
    import cusmc_amd
    from cusmc_amd import _lib, api
    ctx = ctx or api.default_context()
    X = np.ascontiguousarray(X, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    mean, stats = np.empty(d), np.empty(2)
    P = np.empty((d, d)) if cov else None
    entry = _lib.lib().cusmc_moments_log_host if log else _lib.lib().cusmc_moments_host
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _lib.check(entry(ctx._h, p(X), N, ldx, d, p(w), p(mean), p(P), p(stats)))
    return {"mean": mean, "cov": P, "ess": stats[0], "loglik_increment": stats[1]}


def _ratios(got, X, w, log):
    """Worst err / bound of each output (0 for matching degenerate outputs)."""
    ref = MR.moments(X, w, log)
    _, _, state = MR.effective(w, log)
    N, d = X.shape
    if state != "ok":
        assert np.isnan(got["mean"]).all() and np.isnan(got["cov"]).all()
        if state == "none":
            assert got["ess"] == 0.0 and got["loglik_increment"] == -np.inf
        else:
            assert np.isnan(got["ess"]) and got["loglik_increment"] == np.inf
        return 0.0
    s1, s2, am = MR.error_scales(X, w, log)
    assert np.array_equal(got["cov"], got["cov"].T)  # both triangles bitwise equal
    r = []
    bm = CB * U * (s1 + am)
    r.append(np.max(np.abs(got["mean"] - ref["mean"]) / np.where(bm > 0, bm, np.inf), initial=0.0))
    assert np.array_equal(got["mean"][bm == 0], ref["mean"][bm == 0])
    bp = CB * U * s2
    r.append(np.max(np.abs(got["cov"] - ref["cov"]) / np.where(bp > 0, bp, np.inf), initial=0.0))
    assert np.all(got["cov"][bp == 0] == 0.0)
    r.append(abs(got["ess"] - ref["ess"]) / ref["ess"] / (CB * U * max(1.0, math.log2(N))))
    r.append(abs(got["loglik_increment"] - ref["loglik_increment"]) / (CB * U * (1 + abs(ref["loglik_increment"]))))
    return max(r)


DIMS_ALL = [1, 2, 7, 8, 15, 16, 17, 63, 64, 100, 128, 200, 256, 300, 384]


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS_ALL)
def test_standalone_against_the_reference(d):
    """Every weight family at N in {1, 63, 64 +- 1 (the smallest chunk is 64 rows)} and 4097, 1e5 for d <= 17, 257
    above (the long-double reference is the cost), with ldx = d and ldx = d + 3 up to N = 65; at d = 200 and 384
    also N = 6000 for three families: chunks of several LDS stages, and at d = 384 three pair groups.  Worst observed
    err / bound (C = 64) on an MI355X: 0.034 (d = 1), 0.060 (2), 0.063 (7), 0.073 (8), 0.066 (15), 0.113 (16),
    0.128 (17), 0.131 (63), 0.149 (64), 0.125 (100, 128), 0.129 (200), 0.134 (256), 0.156 (300), 0.168 (384)."""
    rng = np.random.default_rng(100 + d)
    worst = 0.0
    Ns = [1, 63, 65, 4097, 100000] if d <= 17 else [1, 63, 65, 257] + ([6000] if d in (200, 384) else [])
    for N in Ns:
        for name, w, log in _families(rng, N):
            if N == 6000 and name not in ("dens", "dominant", "log_nan"):
                continue  # (the long-double reference at d = 384 costs seconds per family)
            far = int(np.argmax(np.nan_to_num(w, nan=-np.inf))) if name == "dominant" else None
            X = _points(rng, N, d, far)
            for pad in (0, 3):
                if pad and N > 70:
                    continue
                Xw = np.zeros((N, d + pad))
                Xw[:, :d] = X
                got = _host(Xw, N, d + pad, d, w, log)
                try:
                    ratio = _ratios(got, X, w, log)
                except AssertionError:
                    raise AssertionError("d=%d N=%d family=%s ldx=%d" % (d, N, name, d + pad))
                assert ratio <= 1.0, (d, N, name, pad, ratio)
                worst = max(worst, ratio)
    print("d=%d worst err/bound %.4f" % (d, worst))


@pytest.mark.gpu
def test_standalone_at_a_million_rows():
    rng = np.random.default_rng(7)
    N, d = 1000000, 64
    X = _points(rng, N, d)
    w = np.exp(-0.5 * rng.standard_normal(N) ** 2)
    got = _host(X, N, d, d, w, False)
    ref = MR.moments(X, w, cov=False)
    s1, _, am = MR.error_scales(X[:, :4], w)
    assert np.all(np.abs(got["mean"][:4] - ref["mean"][:4]) <= CB * U * (s1 + am))
    assert abs(got["ess"] / ref["ess"] - 1) <= CB * U * math.log2(N)
    assert abs(got["loglik_increment"] - ref["loglik_increment"]) <= CB * U * (1 + abs(ref["loglik_increment"]))
    wh = w / w.max()
    Xc = X - got["mean"]
    P = (wh[:, None] * Xc).T @ Xc / wh.sum()  # float64 BLAS: error ~ u sqrt(N) of the scale, far inside
    assert np.max(np.abs(got["cov"] - P) / (np.sqrt(np.outer(np.diag(P), np.diag(P))))) < 1e-10


@pytest.mark.gpu
def test_exact_integer_blocks():
    """Small integers with power-of-two weights: every product and sum is exact, so a misplaced MFMA lane or a
    transposed block shows as a wrong entry (asymmetric data: column j is j + 1 times a row pattern)."""
    for d in (5, 16, 37, 64, 130, 256):
        N = 4096
        rng = np.random.default_rng(d)
        H = rng.integers(-4, 5, size=(N // 2, d)).astype(np.float64) * (np.arange(d) % 5 + 1)
        X = np.concatenate([H, -H])  # column sums exactly 0: the mean is 0 and the centred rows are X itself
        w = np.ones(N)
        got = _host(X, N, d, d, w, False)
        want = X.T @ X / N
        assert np.array_equal(got["mean"], np.zeros(d)), d
        assert np.array_equal(got["cov"], want), d


@pytest.mark.gpu
def test_bitwise_determinism_and_dev_on_a_side_stream():
    import torch
    import cusmc_amd
    from cusmc_amd import api
    rng = np.random.default_rng(3)
    for d in (3, 64, 200):
        N = 200003
        X = _points(rng, N, d)
        lw = -0.5 * rng.standard_normal(N) ** 2 * d
        a = _host(X, N, d, d, lw, True)
        b = _host(X, N, d, d, lw, True)
        for k in ("mean", "cov"):
            assert np.array_equal(a[k], b[k], equal_nan=True)
        assert a["ess"] == b["ess"] and a["loglik_increment"] == b["loglik_increment"]
        ctx = cusmc_amd.Context()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ctx.set_stream(s.cuda_stream)
            Xd = torch.from_numpy(X).cuda()
            wd = torch.from_numpy(lw).cuda()
            m = torch.empty(d, dtype=torch.float64, device="cuda")
            P = torch.empty(d * d, dtype=torch.float64, device="cuda")
            st = torch.empty(2, dtype=torch.float64, device="cuda")
            api.weighted_moments_dev(Xd, wd, m, P, st, log=True, ctx=ctx)
        s.synchronize()
        assert np.array_equal(m.cpu().numpy(), a["mean"])
        assert np.array_equal(P.cpu().numpy().reshape(d, d), a["cov"])
        assert st[0].item() == a["ess"] and st[1].item() == a["loglik_increment"]
        ctx.close()


def _model(d, rng, diag=False, vscale=1.0):
    G = 0.9 * np.eye(d) if diag else 0.9 * np.eye(d) + 0.05 * np.triu(np.ones((d, d)), 1) / d
    return dict(m0=np.zeros(d), C0=np.eye(d), F=np.eye(d), G=G, V=vscale * np.eye(d), W=0.5 * np.eye(d))


def _simulate(mod, T, rng):
    d = len(mod["m0"])
    x = rng.multivariate_normal(mod["m0"], mod["C0"])
    Y = np.zeros((T, d))
    for t in range(1, T):
        x = mod["G"] @ x + rng.multivariate_normal(np.zeros(d), mod["W"])
        Y[t] = mod["F"] @ x + rng.multivariate_normal(np.zeros(d), mod["V"])
    return Y


def _run(N, T, Y, mod, resampler, dist, **kw):
    import cusmc_amd
    d = Y.shape[1]
    return cusmc_amd.run(N, d, T, Y.T, mod["m0"], mod["C0"], mod["F"], mod["G"], mod["V"], mod["W"],
                         4.0 if dist == "mvt" else 0.0, resampler, dist, seed=11, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("resampler", ["metropolis", "stratified"])
@pytest.mark.parametrize("dist", ["mvn", "mvt"])
@pytest.mark.parametrize("d", [2, 8, 16, 64, 200])
def test_filter_summaries_equal_the_standalone_call(resampler, dist, d, monkeypatch):
    """Row t of the summaries is cusmc_moments on (X_t, w_t) of the history the same run returns, bitwise; the
    summaries-only run gives the same summaries, and the history is cusmc_pf_run_host's (run() without summaries)."""
    if d == 8 and dist == "mvt":
        monkeypatch.setenv("CUSMC_PF_CHUNK_BYTES", str(3 * 8 * 4096 * 8))  # the chunked copy-out
    rng = np.random.default_rng(d)
    mod = _model(d, rng)
    N, T = 4096 + 7, 5
    Y = _simulate(mod, T, rng)
    both = _run(N, T, Y, mod, resampler, dist, summaries=True)
    for t in range(T):
        s = _host(both["posterior_x"][t], N, d, d, both["weights"][t], False)
        assert np.array_equal(both["mean"][t], s["mean"]), t
        assert np.array_equal(both["cov"][t], s["cov"]), t
        assert both["ess"][t] == s["ess"], t
        assert both["loglik_increments"][t] == (0.0 if t == 0 else s["loglik_increment"]), t
    assert both["ess"][0] == N and both["loglik_increments"][0] == 0.0
    only = _run(N, T, Y, mod, resampler, dist, summaries=True, history=False)
    assert "weights" not in only and "posterior_x" not in only
    for k in ("mean", "cov", "ess", "loglik_increments"):
        assert np.array_equal(only[k], both[k]), k
    assert only["loglik"] == both["loglik"]
    nocov = _run(N, T, Y, mod, resampler, dist, summaries=True, history=False, summary_cov=False)
    assert "cov" not in nocov
    for k in ("mean", "ess", "loglik_increments"):
        assert np.array_equal(nocov[k], both[k]), k
    plain = _run(N, T, Y, mod, resampler, dist)
    assert np.array_equal(plain["posterior_x"], both["posterior_x"])
    assert np.array_equal(plain["weights"], both["weights"])


@pytest.mark.gpu
@pytest.mark.parametrize("d,resampler", [(2, "stratified"), (8, "stratified"), (16, "stratified"),
                                         (2, "metropolis")])
def test_summaries_track_the_kalman_filter(d, resampler):
    """Linear-Gaussian model, N = 1e6, T = 30, seeded.  m_t within K sqrt(P_jj / ESS_t) of the Kalman mean, P_t
    within K sqrt(2 / ESS_t) relative, sum ell within LTOL of the exact log-likelihood, each at most 1/3 of its
    tolerance.  sqrt(P / ESS_t) is the one-step Monte Carlo scale only: the filter's error accumulates over the
    steps, and observed worst errors in those units were 2.2 (d = 2), 10 (d = 8) and 27 (d = 16) with the
    stratified resampler, 50 with Metropolis (its finite-B bias), hence K = 100 (Metropolis 200).  That the
    growth with d is Monte Carlo error, not a convention shared by the filter and this test, was checked on an
    MI355X at N = 1e4, 1e5, 1e6, two seeds each: the worst mean error in posterior standard deviations falls
    with N (d = 2: 0.04, 0.011, 0.003; d = 8: 0.15-0.20, 0.05-0.13, 0.01-0.03; d = 16: 0.47-0.74, 0.17-0.22,
    0.10-0.31), the same with a diagonal G at d = 16 (0.49-0.95, 0.27-0.50, 0.08-0.12), and its signed average
    over all steps and components is within 0.02 of zero throughout.  The bootstrap filter's error grows with d
    much faster than 1 / sqrt(ESS_t) suggests: the weights are heavy-tailed, so ESS_t overstates the information.
    Observed margins (worst err / tolerance: mean, cov, loglik): d = 2 0.022 / 0.024 / 0.007, d = 8
    0.100 / 0.072 / 0.037, d = 16 0.272 / 0.174 / 0.002, Metropolis d = 2 0.249 / 0.112 / 0.010."""
    K, LTOL = (200.0 if resampler == "metropolis" else 100.0), 1.0
    rng = np.random.default_rng(1000 + d)
    # V = (2 + d/2) I keeps the weights far from degenerate (with V = I the ESS falls to ~10 at d = 16, where
    # sqrt(P / ESS) no longer describes the error); Metropolis runs B = 50 chain steps (its bias at B = 10 is
    # DESIGN.md section 4.7's)
    mod = _model(d, rng, vscale=2.0 + d / 2.0)
    N, T = 1000000, 30
    Y = _simulate(mod, T, rng)
    r = _run(N, T, Y, mod, resampler, "mvn", summaries=True, history=False, B=50)
    M, P, L = MR.kalman(Y, mod["m0"], mod["C0"], mod["F"], mod["G"], mod["V"], mod["W"])
    wm = wp = 0.0
    for t in range(T):
        ess = r["ess"][t]
        sd = np.sqrt(np.diag(P[t]) / ess)
        wm = max(wm, np.max(np.abs(r["mean"][t] - M[t]) / (K * sd)))
        scale = np.sqrt(np.outer(np.diag(P[t]), np.diag(P[t])))
        wp = max(wp, np.max(np.abs(r["cov"][t] - P[t]) / scale) / (K * math.sqrt(2.0 / ess)))
    wl = abs(r["loglik"] - L.sum()) / LTOL
    print("d=%d %s: mean %.3f cov %.3f loglik %.3f (of tolerance); loglik %.4f exact %.4f min ESS %.0f"
          % (d, resampler, wm, wp, wl, r["loglik"], L.sum(), r["ess"].min()))
    assert wm <= 1 / 3 and wp <= 1 / 3 and wl <= 1 / 3


@pytest.mark.gpu
def test_history_free_filter_runs_beyond_the_history_memory():
    """N = 1e6, d = 64, diagonal G: T steps of history would need 1.1 x the device's memory; the history-free
    filter keeps two steps of particles and must finish with finite summaries."""
    import torch
    total = torch.cuda.get_device_properties(0).total_memory
    N, d = 1000000, 64
    T = math.ceil(1.1 * total / (8 * N * d))
    rng = np.random.default_rng(5)
    mod = _model(d, rng, diag=True)
    Y = np.zeros((T, d))  # (observations at the stationary mean)
    r = _run(N, T, Y, mod, "stratified", "mvn", summaries=True, history=False)
    assert r["mean"].shape == (T, d)
    for k in ("mean", "cov", "ess", "loglik_increments"):
        assert np.isfinite(r[k]).all(), k
    assert np.isfinite(r["loglik"])
    print("T = %d steps (history would need %.0f GB)" % (T, 8.0 * N * d * T / 1e9))


@pytest.mark.gpu
def test_cpp_mirror(tmp_path):
    """cusmc::weighted_moments and cusmc::particle_filter_summary, compiled with g++ against the C ABI."""
    src = tmp_path / "moments_mirror.cpp"
    src.write_text(textwrap.dedent(r'''
        #include <cmath>
        #include <cstdio>
        #include <vector>
        #include "cusmc_amd/host/cusmc_host.hpp"
        using namespace cusmc;
        int main() {
          int fails = 0;
          const double X[] = {0, 1, 2, 5, 4, 9};  // rows (0,1), (2,5), (4,9); equal weights
          const double w[] = {0.5, 0.5, 0.5};
          double m[2], P[4], ess, ell;
          weighted_moments(X, 3, 2, w, m, P, &ess, &ell);
          if (m[0] != 2 || m[1] != 5 || std::fabs(P[0] - 8.0 / 3) > 1e-15 || P[1] != P[2] || ess != 3 ||
              std::fabs(ell - std::log(0.5)) > 1e-15) { std::printf("FAIL weighted_moments\n"); ++fails; }
          const int N = 1000, d = 2, T = 4;
          Matrix I = Matrix::Identity(2);
          Vector m0{0, 0};
          std::vector<double> Y(T * d, 0.1), Xh(T * N * d), wh(T * N), mean(T * d), cov(T * d * d), es(T), ll(T);
          std::vector<unsigned> a(T * N);
          particle_filter_summary(Xh.data(), wh.data(), a.data(), mean.data(), cov.data(), es.data(), ll.data(),
                                  Y.data(), I, I, m0, I, I, I, N, d, T, 0.f, "stratified", "mvn", 3);
          std::vector<double> mean2(T * d), ll2(T);
          particle_filter_summary(nullptr, nullptr, nullptr, mean2.data(), nullptr, nullptr, ll2.data(), Y.data(), I,
                                  I, m0, I, I, I, N, d, T, 0.f, "stratified", "mvn", 3);
          double mt[2], Pt[4], et, lt;
          weighted_moments(Xh.data() + (T - 1) * N * d, N, d, wh.data() + (T - 1) * N, mt, Pt, &et, &lt);
          if (mt[0] != mean[(T - 1) * d] || Pt[3] != cov[(T - 1) * 4 + 3] || et != es[T - 1] || lt != ll[T - 1])
            { std::printf("FAIL summary != weighted_moments\n"); ++fails; }
          for (int k = 0; k < T * d; ++k) if (mean2[k] != mean[k]) { std::printf("FAIL history-free\n"); ++fails; break; }
          for (int k = 0; k < T; ++k) if (ll2[k] != ll[k]) { std::printf("FAIL loglik\n"); ++fails; break; }
          std::printf("%s\n", fails ? "FAILED" : "OK");
          return fails != 0;
        }
    '''))
    exe = tmp_path / "moments_mirror"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", ROOT, "-o", str(exe), str(src),
                           "-L" + os.path.join(ROOT, "cusmc_amd"), "-lcusmc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "cusmc_amd")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
