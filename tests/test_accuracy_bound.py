"""CPU side of the accuracy tests (tests/accuracy_bound.py, tests/golden/accuracy.npz).

* Calibration: an emulation of the library's arithmetic -- the host factor of hostla.h through a g++ shim, numpy
  fp64 for W (x - shift), the epilogue and the per-particle Cholesky -- meets the bound on every fixture case with
  a worst ratio <= 1/8.
* Discrimination: the comparator rejects emulations with one float32 rounding on the path, and with nu + d formed
  in double; for every case with kappa <= 10 the bound is at most 1e-11 of max(|lp*|, |lognorm*|).
* Fixture: a few small cases recomputed with mpmath's own LU solver match the stored values."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import accuracy_bound as AB

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return AB.Fixture()


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostla_acc") / "hostla_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "host", "hostla_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.shim_dist_factor.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.shim_dist_factor.restype = ctypes.c_int
    lib.shim_plan_affine.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2
    lib.shim_plan_affine.restype = None
    lib.shim_mvt_log_const.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int]
    lib.shim_mvt_log_const.restype = ctypes.c_double
    return lib


class Emulator:
    """The library's arithmetic on the CPU.  `mutation` rounds one quantity to float32 (W, q, lognorm) or forms
    nu + d in double ("npd_double")."""

    def __init__(self, shim, mutation=None):
        self.shim, self.mutation = shim, mutation
        self._factors = {}

    def factor(self, S):
        key = (S.shape[0], S.tobytes())
        if key not in self._factors:
            n = S.shape[0]
            S = np.ascontiguousarray(S)
            W, ld = np.empty((n, n)), ctypes.c_double()
            assert self.shim.shim_dist_factor(S.ctypes.data, n, W.ctypes.data, ctypes.byref(ld)) == 0
            if self.mutation == "W32":
                W = W.astype(np.float32).astype(np.float64)
            self._factors[key] = (W, ld.value)
        return self._factors[key]

    def npd(self, nu, d):
        return nu + d if self.mutation == "npd_double" else float(np.float32(np.float32(nu) + np.float32(d)))

    def lognorm(self, kind, nu, d, logdet):
        """cusmc_dist_create() / percov_epilogue(); logdet None: without the determinant term"""
        pi = 3.14159265358979323846
        ld = 0.0 if logdet is None else logdet
        if kind == "mvn":
            v = -0.5 * (d * math.log(2.0 * pi) + ld) if logdet is not None else -0.5 * d * math.log(2.0 * pi)
        else:
            v = self.shim.shim_mvt_log_const(nu, self.npd(nu, d), d)
            if logdet is not None:
                v -= 0.5 * ld
        return float(np.float32(v)) if self.mutation == "lognorm32" else v

    def epilogue(self, kind, nu, d, lognorm, q, log):
        if self.mutation == "q32":
            q = q.astype(np.float32).astype(np.float64)
        if kind == "mvn":
            lp = lognorm - 0.5 * q
        else:
            lp = lognorm - 0.5 * self.npd(nu, d) * np.log1p(q * (1.0 / nu))
        return lp if log else np.exp(lp)

    def run(self, fx, case, log=True):
        d, kind, nu = case["d"], case["kind"], case["nu"]
        inp = fx.inputs(case)
        if case["entry"] == "percov":
            return self.percov(inp["X"], inp["mu"], inp["sigma"], kind, nu, log)
        W, logdet = self.factor(fx.sigma(case))
        X = inp["X"]
        if case["entry"] == "pdf_batch":
            Z = (X - inp["mu"]) @ W.T
        elif np.array_equal(inp["F"], np.eye(d)):
            Z = (X - inp["y"]) @ W.T  # plan_affine with F = I: the centred form, shift = y
        else:
            M, b = np.empty((d, d)), np.empty(d)
            F, y = np.ascontiguousarray(inp["F"]), np.ascontiguousarray(inp["y"])
            self.shim.shim_plan_affine(np.ascontiguousarray(W).ctypes.data, F.ctypes.data, y.ctypes.data, d,
                                       M.ctypes.data, b.ctypes.data)
            Z = b + X @ M.T
        q = np.sum(Z * Z, axis=1)
        return self.epilogue(kind, nu, d, self.lognorm(kind, nu, d, logdet), q, log)

    def percov(self, X, mu, S, kind, nu, log):
        """kernels/percov.hip: per-lane Cholesky (column by column), logdet = 2 sum ln L_jj, forward substitution"""
        n, d = X.shape
        L = np.zeros_like(S)
        for j in range(d):
            s = S[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=1)
            L[:, j, j] = np.sqrt(s)
            for r in range(j + 1, d):
                L[:, r, j] = (S[:, r, j] - np.sum(L[:, r, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
        if self.mutation == "W32":
            L = L.astype(np.float32).astype(np.float64)
        ld = 2.0 * np.sum(np.log(np.diagonal(L, axis1=1, axis2=2)), axis=1)
        z = np.zeros((n, d))
        for j in range(d):
            z[:, j] = (X[:, j] - mu[:, j] - np.sum(L[:, j, :j] * z[:, :j], axis=1)) / L[:, j, j]
        q = np.sum(z * z, axis=1)
        ln = self.lognorm(kind, nu, d, None)
        lp = self.epilogue(kind, nu, d, ln, q, True) - 0.5 * ld
        return lp if log else np.exp(lp)


def all_ratios(fx, emu, c):
    """worst err / bound over every case and output form, per case name"""
    out = {}
    for case in fx.cases:
        forms = [True, False] if case["entry"] != "percov" or case["kind"] == "mvn" else [True]
        out[case["name"]] = max(AB.worst(fx, case, emu.run(fx, case, log), log, c)[0] for log in forms)
    return out


def test_fixture_is_consistent(fx):
    """every case has its inputs and references, finite where they must be; the assembly pool has 256 rows"""
    assert len(fx.cases) > 200
    for case in fx.cases:
        ref = fx.ref(case)
        n = len(ref["lp"])
        assert ref["q"].shape == ref["p"].shape == (n,) and np.all(np.isfinite(ref["lp"])), case["name"]
        assert np.all(ref["q"] >= 0.0)
        X = fx.inputs(case)["X"]
        assert X.shape == (n, case["d"])
        if case["entry"] != "percov":
            S = fx.sigma(case)
            assert np.array_equal(S, S.T)
    assert fx.ref(fx.by_name["asm64"])["lp"].shape == (256,)
    entries = {c["entry"] for c in fx.cases}
    assert entries == {"pdf_batch", "reweight", "percov"}
    assert {c["d"] for c in fx.cases} >= {1, 3, 8, 15, 16, 17, 48, 64, 65, 100, 176, 177, 200, 256, 257, 320, 384}
    assert {c["nu"] for c in fx.cases if c["kind"] == "mvt"} >= {0.5, 1.0, 2.5, 4.0, 30.0, 1e4, float(np.float32(3e7))}
    # regimes: exact zeros, tails, subnormal and zero densities
    allq = np.concatenate([fx.ref(c)["q"] for c in fx.cases])
    allp = np.concatenate([fx.ref(c)["p"] for c in fx.cases])
    assert np.any(allq == 0) and np.any(allq < 1e-19) and np.any(allq > 1e99)
    assert np.any((allp > 0) & (allp < 2.0 ** -1022)) and np.any(allp == 0)
    assert max(c.get("kappa", 0.0) for c in fx.cases) > 1e11


def test_input_recipes_are_exact():
    """the fixture's inputs are rebuilt, not stored: the stream is SplitMix64 (its published first output from
    state 0), and every matrix product of the recipes is exact -- summing in the reverse order gives the same bits,
    so no BLAS kernel, thread count or FMA can change an input"""
    assert int(AB.words(0, 1)[0]) == 0xE220A8397B1DCDAF
    u = AB.uniform(AB.key("t"), 4096)
    assert np.all((u >= -1.0) & (u < 1.0)) and len(np.unique(u)) == 4096
    for d in (1, 8, 64, 200, 384):
        M = AB.signs(AB.key("M", d), (d, d))
        for E in AB.GRADED.values():
            lam = np.array([2.0 ** -round(E * k / (d - 1)) for k in range(d)]) if d > 1 else np.ones(1)
            rev = ((M[:, ::-1] * lam[::-1]) @ M[:, ::-1].T) * 2.0 ** -((d - 1).bit_length()) + 2.0 ** -E * np.eye(d)
            assert np.array_equal(AB.graded(M, E), rev), (d, E)
        F = AB.make_F("hard", d, "t") if d > 1 else None
        if F is not None:
            lam = np.array([2.0 ** -round(20 * k / (d - 1)) for k in range(d)])
            M1, M2 = AB.signs(AB.key("F1", "t"), (d, d)), AB.signs(AB.key("F2", "t"), (d, d))
            rev = ((M1[:, ::-1] * lam[::-1]) @ M2[:, ::-1].T) * 2.0 ** -((d - 1).bit_length()) + 2.0 ** -20 * np.eye(d)
            assert np.array_equal(F, rev), d
    for name in ("spd", "g12", "dcd", "sm30", "sp30"):
        S = AB.make_sigma(name, 64)
        assert np.array_equal(S, S.T) and np.all(np.linalg.eigvalsh(S / np.sqrt(np.outer(np.diag(S), np.diag(S)))) > 0)


@pytest.mark.parametrize("name", ["pdf/spd_d1_mvn", "pdf/spd_d3_mvt1", "pdf/g12_d8_mvt0.5", "pdf/dcd_d8_mvn",
                                  "pdf/sm30_d8_mvt4", "reweight_F/spd_d8_hard_mvt4", "percov/d3_mvt"])
def test_fixture_matches_mpmath(fx, name):
    """an independent recomputation: mpmath's LU solve and determinant at 50 digits, straight from the fp64 inputs"""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone() if hasattr(mpmath.mp, "clone") else mpmath.mp
    mp.dps = 50
    case = fx.by_name[name]
    d, kind, nu = case["d"], case["kind"], case["nu"]
    inp, ref = fx.inputs(case), fx.ref(case)
    npd = mp.mpf(float(np.float32(np.float32(nu) + np.float32(d))))
    for i, x in enumerate(inp["X"]):
        if case["entry"] == "percov":
            S, r = inp["sigma"][i], [mp.mpf(a) - mp.mpf(b) for a, b in zip(x, inp["mu"][i])]
        elif case["entry"] == "pdf_batch":
            S, r = fx.sigma(case), [mp.mpf(a) - mp.mpf(b) for a, b in zip(x, inp["mu"])]
        else:
            S = fx.sigma(case)
            r = [mp.mpf(inp["y"][k]) - mp.fsum(mp.mpf(inp["F"][k][j]) * mp.mpf(x[j]) for j in range(d))
                 for k in range(d)]
        Sm = mp.matrix([[mp.mpf(v) for v in row] for row in S])
        rv = mp.matrix(r)
        q = (rv.T * mp.lu_solve(Sm, rv))[0] if any(r) else mp.mpf(0)
        logdet = mp.log(mp.det(Sm))
        if kind == "mvn":
            lp = -(d * mp.log(2 * mp.pi) + logdet) / 2 - q / 2
        else:
            mn = mp.mpf(nu)
            lp = (mp.loggamma(npd / 2) - mp.loggamma(mn / 2) - d * mp.log(mp.pi * mn) / 2 - logdet / 2
                  - npd / 2 * mp.log1p(q / mn))
        assert abs(float(lp) - ref["lp"][i]) <= 2.0 ** -52 * abs(ref["lp"][i]), (name, i)
        assert abs(float(q) - ref["q"][i]) <= 2.0 ** -50 * ref["q"][i], (name, i)


def test_calibration(fx, shim):
    """the library's arithmetic, emulated, meets the bound with a worst ratio <= 1/8 at the recorded C"""
    emu = Emulator(shim)
    r = all_ratios(fx, emu, 1.0)
    worst_name = max(r, key=r.get)
    print("calibration: worst err/bound at C = 1: %.3g (%s)" % (r[worst_name], worst_name))
    assert AB.C is not None and AB.CALIBRATED_WORST is not None
    assert r[worst_name] <= AB.CALIBRATED_WORST, (worst_name, r[worst_name])
    assert AB.CALIBRATED_WORST * 8.0 <= AB.C
    assert max(all_ratios(fx, emu, AB.C).values()) <= 1.0 / 8.0


@pytest.mark.parametrize("mutation", ["W32", "q32", "lognorm32", "npd_double"])
def test_mutations_are_rejected(fx, shim, mutation):
    """one float32 rounding on the path, or nu + d formed in double, exceeds the bound on at least one case"""
    emu = Emulator(shim, mutation)
    r = all_ratios(fx, emu, AB.C)
    assert max(r.values()) > 1.0, "mutation %s passes every case" % mutation


def test_bound_is_tight_when_well_conditioned(fx):
    """kappa <= 10: the bound is at most 1e-11 of the size of the terms lp* is formed from, max(|lp*|, |lognorm*|) --
    a flat 1e-6 relative tolerance cannot tell fp64 from fp32.  (Relative to |lp*| alone no fp64 evaluation could
    meet it on the rows where lognorm* - q*/2 cancels, e.g. the subnormal density of a covariance scaled by 1e-30.)"""
    for case in fx.cases:
        ref = fx.ref(case)
        sel = AB.kappa_of(fx, case) <= 10.0
        size = np.maximum(np.abs(ref["lp"]), np.abs(ref["lognorm"]))
        assert np.all(AB.bound(fx, case)[sel] <= 1e-11 * size[sel]), case["name"]


def test_mvt_normalising_constant(fx, shim):
    """the library's Student-t constant (hostla.h mvt_log_const) against mpmath, nu up to 3e7: the plain
    lgamma((nu+d)/2) - lgamma(nu/2) - d/2 log(pi nu) was off by up to 4e-8 at nu = 3e7"""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    for nu in (0.5, 1.0, 2.5, 4.0, 30.0, 31.0, 32.0, 33.0, 1e3, 1e4, 3e7, 1e9):
        for d in (1, 2, 3, 16, 17, 64, 65, 384):
            nu32 = float(np.float32(nu))
            npd = float(np.float32(np.float32(nu32) + np.float32(d)))
            got = shim.shim_mvt_log_const(nu32, npd, d)
            want = (mpmath.loggamma(mpmath.mpf(npd) / 2) - mpmath.loggamma(mpmath.mpf(nu32) / 2)
                    - d * mpmath.log(mpmath.pi * nu32) / 2)
            assert abs(got - float(want)) <= 8 * AB.U * (abs(float(want)) + d), (nu, d, got, float(want))
