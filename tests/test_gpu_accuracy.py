"""Every log-density entry point against the extended-precision references of tests/golden/accuracy.npz, each element
held to the conditioning-scaled bound of tests/accuracy_bound.py (C fixed on the CPU by tests/test_accuracy_bound.py).

Kernel families (run_logpdf, cusmc_abi.hip): small (d < 16), matrix-core (16 <= d <= 176; padded when d % 16, or an
odd or misaligned row stride), wide (176 < d <= 256), generic (d > 256), the d = 64 assembly kernel (MVN, mu = 0,
contiguous, N >= 16 tiles per CU), the per-particle covariance kernels (percov.hip) and the QL-rotated general-F
reweight.  The worst err/bound per family is printed by test_zz_report (pytest -s)."""
import collections

import numpy as np
import pytest

import accuracy_bound as AB

pytestmark = pytest.mark.gpu

FX = AB.Fixture()
WORST = collections.defaultdict(float)


def _note(fam, w):
    WORST[fam] = max(WORST[fam], w)


@pytest.fixture(scope="module")
def cs():
    import cusmc_amd
    return cusmc_amd


def _dist(cs, case, mu, S):
    if case["kind"] == "mvn":
        return cs.MultiVariateNormalDistribution(mu, S)
    return cs.MultiVariateTStudentDistribution(mu, S, case["nu"])


def _ids(cases):
    return [c["name"] for c in cases]


PDF = FX.select("pdf_batch")
REWEIGHT = FX.select("reweight")
PERCOV = FX.select("percov")


@pytest.mark.parametrize("case", PDF, ids=_ids(PDF))
def test_pdf_batch(cs, case):
    inp = FX.inputs(case)
    D = _dist(cs, case, inp["mu"], FX.sigma(case))
    try:
        for log in (True, False):
            _note(AB.family(case["d"]), AB.check(FX, case, D.pdf_batch(inp["X"], log=log), log))
    finally:
        D.close()


@pytest.mark.parametrize("case", REWEIGHT, ids=_ids(REWEIGHT))
def test_reweight(cs, case):
    inp = FX.inputs(case)
    d = case["d"]
    D = _dist(cs, case, np.zeros(d), FX.sigma(case))
    general = not np.array_equal(inp["F"], np.eye(d))
    fam = "general-F reweight (%s)" % ("dense" if d < 16 else "QL") if general else AB.family(d)
    try:
        for log in (True, False):
            _note(fam, AB.check(FX, case, D.reweight(inp["X"], inp["y"], inp["F"], log=log), log))
    finally:
        D.close()


@pytest.mark.parametrize("case", PERCOV, ids=_ids(PERCOV))
def test_logpdf_percov(cs, case):
    inp = FX.inputs(case)
    nu = None if case["kind"] == "mvn" else case["nu"]
    forms = (True, False) if nu is None else (True,)
    for log in forms:
        got, info = cs.logpdf_percov(inp["X"], inp["mu"], inp["sigma"], nu=nu, log=log)
        assert np.all(info == 0)
        _note("percov", AB.check(FX, case, got, log))


@pytest.mark.parametrize("d", range(1, 17))
def test_cholesky_batched_logdet(cs, d):
    """logdet of the batched device Cholesky: |ld - ld*| <= C u (|ld*| + d kappa), kappa per covariance"""
    case = FX.by_name["percov/d%d_mvn" % d]
    inp = FX.inputs(case)
    L, ld, info = cs.cholesky_batched(inp["sigma"])
    assert np.all(info == 0)
    want = inp["logdet"]
    b = AB.C * AB.U * (np.abs(want) + d * inp["kappa"])
    r = np.abs(ld - want) / b
    assert np.all(np.isfinite(ld)) and r.max() <= 1.0, "d = %d: worst err/bound %.3g" % (d, r.max())
    _note("percov (cholesky_batched logdet)", float(r.max()))


STRIDED = [c for c in PDF if c["name"] in ["pdf/spd_d%d_%s" % (d, k) for d in (8, 17, 64, 200, 320)
                                           for k in ("mvn", "mvt4", "mvt0.5", "mvt2.5", "mvt30")]
           or c["name"] in ("pdf/g12_d64_mvn", "pdf/dcd_d200_mvt4", "pdf/g12_d384_mvn")]


@pytest.mark.parametrize("parity", ["odd", "even"])
@pytest.mark.parametrize("case", STRIDED, ids=_ids(STRIDED))
def test_pdf_strided(cs, case, parity):
    """rows with ldx > d (NaN in the gap): an odd ldx takes the padded variants, an even one the row-gap path"""
    import torch
    inp = FX.inputs(case)
    d = case["d"]
    ldx = d + 1 if (d + 1) % 2 == (1 if parity == "odd" else 0) else d + 2
    X = inp["X"]
    buf = torch.full((X.shape[0], ldx), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :d] = torch.from_numpy(X).cuda()
    out = torch.empty(X.shape[0], dtype=torch.float64, device="cuda")
    D = _dist(cs, case, inp["mu"], FX.sigma(case))
    try:
        D.ctx.use_torch_stream()
        for log in (True, False):
            D.pdf_dev(buf[:, :d], out, log=log)
            torch.cuda.synchronize()
            _note(AB.family(d, ldx) + " (ldx > d)", AB.check(FX, case, out.cpu().numpy(), log, " ldx=%d" % ldx))
    finally:
        D.close()


@pytest.mark.parametrize("N", [65_536 + 5, 262_144 + 5])
def test_assembly_kernel(cs, N):
    """d = 64, MVN, mu = 0, contiguous, N >= 16 tiles per CU: the assembly kernel.  The rows repeat the 256-row pool
    in a fixed permutation, so every row -- the tail pool's and the last tile's included -- has its reference.
    The same rows in pieces below the threshold (the compiled kernel) meet the bound too, and agree bitwise."""
    import torch
    case = FX.by_name["asm64"]
    inp, ref = FX.inputs(case), FX.ref(case)
    idx = np.random.default_rng(N).permutation(N) % 256
    X = torch.from_numpy(inp["X"][idx]).cuda()
    bound = AB.bound(FX, case)[idx]
    D = cs.MultiVariateNormalDistribution(None, FX.sigma(case))
    try:
        D.ctx.use_torch_stream()
        out = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        D.pdf_dev(X, out)
        pieces = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        for lo in range(0, N, 60_000):  # (< 16 rounds of 256 tiles: the compiled kernel)
            D.pdf_dev(X[lo:lo + 60_000], pieces[lo:lo + 60_000])
        torch.cuda.synchronize()
        for label, got in (("assembly", out.cpu().numpy()), ("matrix-core (asm rows, pieces)", pieces.cpu().numpy())):
            r = np.abs(got - ref["lp"][idx]) / bound
            r = np.where(np.isfinite(got), r, np.inf)
            i = int(np.argmax(r))
            assert r[i] <= 1.0, "%s N=%d: worst err/bound %.3g at row %d (pool row %d)" % (label, N, r[i], i, idx[i])
            _note(label, float(r[i]))
        assert torch.equal(out, pieces)
    finally:
        D.close()


def test_zz_report():
    """the worst err/bound per kernel family over the tests above (printed; pytest -s shows it)"""
    for fam in sorted(WORST):
        print("accuracy: %-40s worst err/bound %.3g" % (fam, WORST[fam]))
