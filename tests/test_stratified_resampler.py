"""The stratified resampler (include/cusmc_hip.h): the CPU restatement's own laws, the C ABI
surface without a GPU, and -- on an MI355X (-m gpu) -- bit-exact ancestors against the restatement, alone and
inside the filter."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, spd
import stratified_ref as R

NAMES = ["cusmc_stratified_dev", "cusmc_stratified_host", "cusmc_stratified_log_dev", "cusmc_stratified_log_host",
         "cusmc_stratified_multi_host"]


def _copies(a, N):
    return np.bincount(a.astype(np.int64), minlength=N)


def _families(rng, N):
    """weight families: (name, weights, log form?)"""
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
    lw_nan = lw - 800.0  # (densities would underflow: the log form's reason to be)
    lw_nan[rng.random(N) < 0.1] = np.nan
    return [("dens", dens, False), ("zeros", zeros, False), ("neg", neg, False), ("nan", nan, False),
            ("equal", np.full(N, 0.25), False), ("dominant", dominant, False),
            ("all_zero", np.zeros(N), False), ("pinf", np.where(np.arange(N) == N // 2, np.inf, dens), False),
            ("all_nan", np.full(N, np.nan), False),
            ("log", lw, True), ("log_minf", lw_inf, True), ("log_nan", lw_nan, True),
            ("log_all_minf", np.full(N, -np.inf), True), ("log_pinf", np.where(np.arange(N) == 0, np.inf, lw), True)]


# --- the restatement (CPU) ------------------------------------------------------------------------------------

def test_numpy_philox_equals_the_oracle(oracle):
    rng = np.random.default_rng(1)
    for _ in range(200):
        ctr = rng.integers(0, 2 ** 32, size=4, dtype=np.uint64).astype(np.uint32)
        key = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64).astype(np.uint32)
        got = np.array(R.philox4x32_10(*ctr, *key), dtype=np.uint32)
        assert np.array_equal(got, oracle.philox4x32_10(ctr, key))


@pytest.mark.parametrize("N", [1, 2, 3, 64, 1000, 4097])
def test_copy_counts_are_within_two_of_their_expectation(N):
    rng = np.random.default_rng(N)
    for name, w, log in _families(rng, N):
        q, degenerate = R.quantised(w, log)
        a = R.stratified(w, seed=99, step=3, log=log)
        assert np.all(np.diff(a.astype(np.int64)) >= 0), name
        if degenerate:
            assert np.array_equal(a, np.arange(N, dtype=np.uint32)), name
            continue
        S = float(q.astype(np.float64).sum())
        o = _copies(a, N)
        assert np.all(np.abs(o - N * q.astype(np.float64) / S) <= 2), name
        assert np.all(o[q == 0] == 0), name  # zero, negative, NaN and -inf weights are never chosen


def test_degenerate_inputs_give_the_identity():
    for w, log in (([0.0, 0.0, 0.0], False), ([-1.0, 0.0], False), ([np.nan] * 5, False), ([1.0, np.inf], False),
                   ([-np.inf, -np.inf], True), ([np.nan, np.nan], True), ([0.0, np.inf], True)):
        a = R.stratified(np.array(w), seed=1, step=1, log=log, first=0)
        assert np.array_equal(a, np.arange(len(w), dtype=np.uint32))
    assert np.array_equal(R.stratified(np.zeros(10), 1, first=4, count=3), [4, 5, 6])


def test_mean_copy_count_matches_the_weights():
    N = 50
    rng = np.random.default_rng(5)
    w = rng.exponential(size=N) ** 3
    w[[3, 17]] = 0.0
    q, _ = R.quantised(w)
    want = N * q.astype(np.float64) / float(q.astype(np.float64).sum())
    seeds = 2000
    tot = np.zeros(N)
    for s in range(seeds):
        tot += _copies(R.stratified(w, seed=1000 + s, step=1), N)
    mean = tot / seeds
    # a count stays within two of its expectation: its standard deviation is below 2
    assert np.all(np.abs(mean - want) <= 5 * 2 / np.sqrt(seeds))
    assert np.abs(mean - want).max() < 0.1
    assert mean[3] == 0 and mean[17] == 0


# --- the C ABI without a GPU ----------------------------------------------------------------------------------

def _declared():
    text = open(os.path.join(ROOT, "include", "cusmc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(cusmc_[a-z0-9_]+)\s*\(", text))


def test_header_declares_and_ctypes_binds_the_stratified_entries():
    from cusmc_amd import _lib
    declared = _declared()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    L = _lib.lib()
    for name in NAMES:
        assert name in declared and name in bound
        assert hasattr(L, name)


def _has_gpu():
    from cusmc_amd import _lib
    return _lib.lib().cusmc_device_count() > 0


def test_entries_validate_and_refuse_without_a_device():
    import cusmc_amd
    from cusmc_amd import _lib
    L = _lib.lib()
    w = np.ones(4)
    a = np.zeros(4, dtype=np.uint32)
    devs = (C.c_int * 1)(0)
    # argument checks come first, on any box
    assert L.cusmc_stratified_multi_host(devs, 1, None, 4, 1, 1, 0, a.ctypes.data) == _lib.EINVAL
    assert L.cusmc_stratified_multi_host(devs, 1, w.ctypes.data, 0, 1, 1, 0, a.ctypes.data) == _lib.EINVAL
    assert L.cusmc_stratified_dev(None, None, 4, 1, 1, 0, 4, None) == _lib.EINVAL
    I = np.eye(2)
    with pytest.raises(cusmc_amd.CusmcError) as e:  # the sharded filter refuses the stratified resampler
        cusmc_amd.run(8, 2, 3, np.zeros((2, 3)), np.zeros(2), I, I, I, I, I, 0.0, "stratified", "mvn", seed=1,
                      devices=[0, 0])
    assert e.value.code == _lib.EINVAL and "stratified" in str(e.value)
    with pytest.raises(cusmc_amd.CusmcError) as e:
        cusmc_amd.run(8, 2, 3, np.zeros((2, 3)), np.zeros(2), I, I, I, I, I, 0.0, "systematic", "mvn", seed=1,
                      devices=[0, 0])
    assert e.value.code == _lib.EINVAL and "metropolis, stratified" in str(e.value)
    if _has_gpu():
        return
    assert L.cusmc_stratified_multi_host(devs, 1, w.ctypes.data, 4, 1, 1, 0, a.ctypes.data) == _lib.ENODEVICE
    for call in (lambda: cusmc_amd.Sampler.stratified(w), lambda: cusmc_amd.Sampler.stratified_log(np.log(w)),
                 lambda: cusmc_amd.Sampler.stratified(w, devices=[0])):
        with pytest.raises(cusmc_amd.CusmcError) as e:
            call()
        assert e.value.code == _lib.ENODEVICE


# --- on the GPU -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cs():
    import cusmc_amd
    from cusmc_amd import _lib
    assert _lib.lib().cusmc_device_count() > 0, "no GPU visible: the gpu suite needs an MI355X"
    return cusmc_amd


def _mismatch(got, want):
    bad = np.flatnonzero(got != want)
    return "%d of %d differ (first at %s: %s vs %s)" % (bad.size, want.size, bad[:3], got[bad[:3]], want[bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3, 64, 1000, 4097, 100_003, 2 ** 20])
def test_ancestors_are_bit_exact(cs, N):
    rng = np.random.default_rng(N + 11)
    fams = _families(rng, N)
    if N == 2 ** 20:  # (the log families' restatement evaluates exp element by element: keep the big case lean)
        fams = [f for f in fams if f[0] in ("dens", "zeros", "dominant", "log_minf")]
    for name, w, log in fams:
        for seed, step in ((1, 1), (0xDEADBEEF12345678, 7)):
            f = cs.Sampler.stratified_log if log else cs.Sampler.stratified
            got = f(w, seed=seed, t=step)
            want = R.stratified(w, seed, step, log=log)
            assert np.array_equal(got, want), (name, seed, step, _mismatch(got, want))


@pytest.mark.gpu
def test_shards_compose_on_the_device(cs):
    import torch
    N = 50_000
    rng = np.random.default_rng(3)
    for name, w, log in _families(rng, N)[:6] + _families(rng, N)[9:11]:
        wd = torch.from_numpy(w).cuda()
        want = R.stratified(w, 5, 2, log=log)
        whole = torch.empty(N, dtype=torch.int32, device="cuda")
        cs.Sampler.stratified_dev(wd, whole, t=2, seed=5, log=log)
        assert np.array_equal(whole.cpu().numpy().view(np.uint32), want), name
        parts = []
        for first, count in ((0, 1), (1, 2047), (2048, 2049), (4097, 12345), (16442, N - 16442)):
            a = torch.empty(count, dtype=torch.int32, device="cuda")
            cs.Sampler.stratified_dev(wd, a, t=2, seed=5, first=first, log=log)
            parts.append(a.cpu().numpy().view(np.uint32))
        assert np.array_equal(np.concatenate(parts), want), name
    if log:
        a = torch.empty(10, dtype=torch.int32, device="cuda")
        cs.Sampler.stratified_log_dev(wd, a, t=2, seed=5, first=100)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), want[100:110])


@pytest.mark.gpu
def test_device_entries_validate(cs):
    import torch
    from cusmc_amd import _lib
    L = _lib.lib()
    ctx = cs.api.default_context()
    w = torch.ones(8, dtype=torch.float64, device="cuda")
    a = torch.empty(8, dtype=torch.int32, device="cuda")
    assert L.cusmc_stratified_dev(ctx._h, C.c_void_p(w.data_ptr()), 0, 1, 1, 0, 0, C.c_void_p(a.data_ptr())) == _lib.EINVAL
    assert L.cusmc_stratified_dev(ctx._h, C.c_void_p(w.data_ptr()), 8, 1, 1, 4, 5, C.c_void_p(a.data_ptr())) == _lib.EINVAL
    assert L.cusmc_stratified_log_dev(ctx._h, None, 8, 1, 1, 0, 8, C.c_void_p(a.data_ptr())) == _lib.EINVAL
    assert L.cusmc_stratified_host(ctx._h, None, 8, 1, 1, None) == _lib.EINVAL


@pytest.mark.gpu
def test_one_million_subset_and_copy_bound(cs):
    N = 1_000_000
    rng = np.random.default_rng(8)
    x = rng.standard_normal((N, 2))
    w = np.exp(-0.5 * (x ** 2).sum(1) / 0.05)
    got = cs.Sampler.stratified(w, seed=77, t=4)
    idx = np.sort(rng.choice(N, 4000, replace=False))
    want = R.stratified(w, 77, 4)  # (whole vector: the subset below is keyed by the global index)
    assert np.array_equal(got[idx], want[idx])
    for i in idx[:50]:
        assert R.stratified(w, 77, 4, first=int(i), count=1)[0] == got[i]
    q, _ = R.quantised(w)
    o = _copies(got, N)
    assert np.all(np.abs(o - N * q.astype(np.float64) / float(q.astype(np.float64).sum())) <= 2)


@pytest.mark.gpu
def test_multi_host_equals_one_device(cs):
    rng = np.random.default_rng(21)
    for N in (1, 2, 5, 1000, 100_003):
        for name, w, log in _families(rng, N)[:4] + _families(rng, N)[9:11]:
            one = (cs.Sampler.stratified_log if log else cs.Sampler.stratified)(w, seed=9, t=3)
            multi = (cs.Sampler.stratified_log if log else cs.Sampler.stratified)(w, seed=9, t=3, devices=[0, 0, 0])
            assert np.array_equal(one, multi), (N, name)


def _model(rng, d):
    G = 0.9 * np.eye(d) + 0.05 * rng.standard_normal((d, d)) / np.sqrt(max(d, 8) / 8)
    F = np.eye(d) + 0.05 * rng.standard_normal((d, d)) / np.sqrt(max(d, 8) / 8)
    return G, F, spd(rng, d), 0.3 * spd(rng, d), spd(rng, d), rng.standard_normal(d)


@pytest.mark.gpu
@pytest.mark.parametrize("d,dist,nu", [(2, "mvn", 0.0), (2, "mvt", 5.0), (8, "mvn", 0.0), (8, "mvt", 5.0),
                                       (64, "mvn", 0.0), (64, "mvt", 5.0)])
def test_filter_with_the_stratified_resampler(cs, oracle, d, dist, nu):
    """run(..., "stratified"): every step's ancestors are the restatement's over the returned w_{t-1}, and the
    proposal and the weights are the oracle's step functions applied to them."""
    rng = np.random.default_rng(60 + d)
    T, N = (6, 3000) if d <= 8 else (4, 700)
    G, F, V, W, C0, m0 = _model(rng, d)
    Y = rng.standard_normal((T, d))
    seed = 4242
    out = cs.run(N, d, T, Y.T, m0, C0, F, G, V, W, nu, "stratified", dist, seed=seed, return_ancestors=True)
    X, w, a = out["posterior_x"], out["weights"], out["ancestors"]
    Qw = oracle.eigen_sqrt(W)
    for t in range(1, T):
        want = R.stratified(w[t - 1], seed, t)
        assert np.array_equal(a[t], want), (t, _mismatch(a[t], want))
        assert np.allclose(X[t], oracle.propagate(X[t - 1], a[t], G, Qw, dist, nu, 1.0, seed=seed, step=t),
                           rtol=1e-8, atol=1e-8), t
        assert np.allclose(w[t], oracle.reweight(X[t], Y[t], F, V, dist, nu), rtol=1e-6, atol=1e-300), t


@pytest.mark.gpu
def test_stratified_filter_tracks_a_linear_gaussian_state(cs):
    """Statistical sanity at a real size: the filter mean follows the Kalman mean."""
    rng = np.random.default_rng(0)
    d, T, N = 2, 30, 200_000
    I = np.eye(d)
    V, W = 0.5 * I, 0.1 * I
    x = np.zeros(d)
    Y = np.zeros((T, d))
    for t in range(1, T):
        x = x + rng.multivariate_normal(np.zeros(d), W)
        Y[t] = x + rng.multivariate_normal(np.zeros(d), V)
    out = cs.run(N, d, T, Y.T, np.zeros(d), I, I, I, V, W, 0.0, "stratified", "mvn", seed=3)
    m, P = np.zeros(d), I.copy()
    for t in range(1, T):
        P = P + W
        K = P @ np.linalg.inv(P + V)
        m = m + K @ (Y[t] - m)
        P = (I - K) @ P
    w = out["weights"][-1]
    est = (out["posterior_x"][-1] * w[:, None]).sum(0) / w.sum()
    assert np.allclose(est, m, atol=0.05)
