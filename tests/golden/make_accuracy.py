"""Generates tests/golden/accuracy.npz: log-densities with extended-precision references.

    python tests/golden/make_accuracy.py

Every fp64 input (Sigma, mu, x, y, F) is taken as exact.  The linear algebra runs in exact fixed point on Python
integers with a resolution of 2^-300 after an exact power-of-two diagonal equilibration; logarithms, lgamma and
the final rounding run in mpmath at 60 digits.  A stored value is the fp64 rounding of a quantity known to ~80
digits: correctly rounded.  Student-t follows the library's float semantics: nu is a float32 value and nu + d is
formed in float32, both inside lgamma and in the (nu + d) / 2 factor of the epilogue.  No library code is used.

Layout (tests/accuracy_bound.py reads it): `meta` holds {"cases": [...], "inputs": {row set: recipe}}.  No input
array is stored: tests/accuracy_bound.py rebuilds Sigma, F, mu, y and X bit for bit from the recipes (+-1 matrices,
powers of two and a SplitMix64 stream: exact on every machine), with "in/<row set>/c" the per-row scales (and, for
percov, the exponents E, t and the exact logdet and kappa per covariance).  Per case "<case>/{lp,p,q,lognorm}":
log-density, density (subnormals and 0 included), q = |L^-1 r|^2 and the normalising constant; `meta` also gives
kappa2 = kappa_2(Sigma) and kappa = kappa_2 of Sigma scaled to unit diagonal (fp64 singular values of the exact
factor).

Cases
  pdf_batch   every dispatch route of the log-pdf kernels (d = 1 .. 384); well-conditioned covariances at every d;
              graded spectra (kappa ~1e4, 1e8, 1e12), D C D with D over 1e-8 .. 3e8, overall scales 1e-30 / 1e30 at
              d = 8, 64, 200, 384; residuals with q = 0, 1e-20, d, 1e6, 1e100 and one whose MVN density is
              subnormal; a mean 1e8 away from the origin.  MVN, and Student-t with nu in {0.5, 1, 2.5, 4, 30, 1e4, 3e7}.
  reweight    F = I, and general F (kappa(F) <~ 10 and ~ 1e6) on the dense (d < 16) and QL-rotated paths, r = y - F x.
  percov      d = 1 .. 16, one covariance per particle, kappa over 1 .. 1e10.
  asm64       256 rows of one d = 64, mu = 0 case: the pool the assembly-kernel test repeats.
"""
import json
import math
import os
import sys
import time

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import accuracy_bound as AB  # noqa: E402  (the input recipes; numpy only)
OUT = os.path.join(HERE, "accuracy.npz")

P = 300  # fixed-point fraction bits
mpmath.mp.dps = 60
TWO_P = mpmath.mpf(2) ** P

DIMS = [1, 3, 8, 15, 16, 17, 48, 64, 65, 100, 176, 177, 200, 256, 257, 320, 384]
HARD_DIMS = [8, 64, 200, 384]
NUS = [0.5, 1.0, 2.5, 4.0, 30.0, 1e4, 3e7]


# ---- exact arithmetic ---------------------------------------------------------------------------------------------
# A dyadic number is (n, k) with value n * 2^k; every finite float is one.

def dyadic(v):
    n, m = float(v).as_integer_ratio()
    return n, -(m.bit_length() - 1)


def dy_sum(terms):
    terms = [t for t in terms if t[0]]
    if not terms:
        return 0, 0
    k = min(t[1] for t in terms)
    return sum(n << (e - k) for n, e in terms), k


def dy_sub(a, b):
    return dy_sum([a, (-b[0], b[1])])


def dy_fixed(a, shift):
    """floor(a * 2^(P - shift))"""
    n, k = a
    e = k + P - shift
    return n << e if e >= 0 else n >> -e


def dy_abs_log2(a):
    n, k = a
    return n.bit_length() + k if n else None


class ExactFactor:
    """Sigma = E Lt Lt^T E with E = diag(2^e_i) (exact), Lt lower triangular in fixed point (ints scaled by 2^P)."""

    def __init__(self, S):
        d = self.d = S.shape[0]
        self.e = [int(round(0.5 * math.log2(S[i, i]))) for i in range(d)]
        L = [[0] * d for _ in range(d)]
        for j in range(d):
            Lj = L[j]
            s = dy_fixed(dyadic(S[j, j]), 2 * self.e[j]) - (sum(v * v for v in Lj[:j]) >> P)
            if s <= 0:
                raise ValueError("not positive definite at pivot %d" % j)
            ljj = Lj[j] = math.isqrt(s << P)
            for i in range(j + 1, d):
                Li = L[i]
                t = (dy_fixed(dyadic(S[i, j]), self.e[i] + self.e[j]) << P) - sum(a * b for a, b in zip(Li[:j], Lj[:j]))
                Li[j] = t // ljj
        self.L = L

    def logdet(self):
        s = mpmath.mpf(0)
        for j in range(self.d):
            s += mpmath.log(mpmath.mpf(self.L[j][j]) / TWO_P) + self.e[j] * mpmath.log(2)
        return 2 * s

    def q(self, r):
        """|L^-1 r|^2 for an exact residual r (list of dyadics), as mpf."""
        mags = [dy_abs_log2(v) for v in r]
        mags = [m - self.e[i] for i, m in enumerate(mags) if m is not None]
        if not mags:
            return mpmath.mpf(0)
        sr = max(mags)
        z = []
        for j in range(self.d):
            Lj = self.L[j]
            t = (dy_fixed(r[j], self.e[j] + sr) << P) - sum(a * b for a, b in zip(Lj[:j], z))
            z.append(t // Lj[j])
        return mpmath.mpf(sum(v * v for v in z)) * mpmath.mpf(2) ** (2 * sr - 2 * P)

    def kappa(self):
        Lf = np.array([[float(mpmath.mpf(v) / TWO_P) for v in row] for row in self.L])
        E = np.array([2.0 ** e for e in self.e])
        sv = np.linalg.svd(E[:, None] * Lf, compute_uv=False)
        k2 = float(sv[0] / sv[-1]) ** 2
        sv = np.linalg.svd(Lf / np.sqrt(np.sum(Lf * Lf, axis=1))[:, None], compute_uv=False)
        return k2, float(sv[0] / sv[-1]) ** 2


def residual_centred(x, mu):
    return [dy_sub(dyadic(a), dyadic(b)) for a, b in zip(x, mu)]


def residual_affine(y, F, x):
    xd = [dyadic(v) for v in x]
    out = []
    for i in range(len(y)):
        terms = [dyadic(y[i])]
        for j, fv in enumerate(F[i]):
            n, k = dyadic(fv)
            terms.append((-n * xd[j][0], k + xd[j][1]))
        out.append(dy_sum(terms))
    return out


def npd32(nu32, d):
    return mpmath.mpf(float(np.float32(np.float32(nu32) + np.float32(d))))


def lognorm_exact(kind, d, nu32, logdet):
    pi = mpmath.pi
    if kind == "mvn":
        return -(d * mpmath.log(2 * pi) + logdet) / 2
    nu = mpmath.mpf(nu32)
    return mpmath.loggamma(npd32(nu32, d) / 2) - mpmath.loggamma(nu / 2) - d * mpmath.log(pi * nu) / 2 - logdet / 2


def lp_exact(kind, d, nu32, lognorm, q):
    if kind == "mvn":
        return lognorm - q / 2
    return lognorm - npd32(nu32, d) / 2 * mpmath.log1p(q / mpmath.mpf(nu32))


def round_density(lp):
    """exp(lp) correctly rounded to fp64, subnormals and 0 included."""
    v = mpmath.exp(lp)
    if v >= mpmath.mpf(2) ** -1022:
        return float(v)
    return math.ldexp(int(mpmath.nint(v * mpmath.mpf(2) ** 1074)), -1074)


# ---- inputs -------------------------------------------------------------------------------------------------------
# The recipes (tests/accuracy_bound.py) rebuild every input bit for bit from a few stored numbers; what is stored per
# row set is the row scale c_j (X_j = base + c_j u_j), chosen here so that q lands near the wanted regime.

def row_scales(S, U, targets):
    """c_j with c_j^2 u_j^T S^-1 u_j ~ target_j (fp64 is plenty: only the regime matters, q* is computed exactly)"""
    Sinv_u = np.linalg.solve(S, U.T).T
    qu = np.sum(U * Sinv_u, axis=1)
    return np.array([0.0 if t == 0 else math.sqrt(t / v) for t, v in zip(targets, qu)])


class Writer:
    def __init__(self):
        self.arrays, self.cases, self.specs, self.factors = {}, [], {}, {}

    def factor(self, sname, d):
        key = (sname, d)
        if key not in self.factors:
            S = AB.make_sigma(sname, d)
            assert np.array_equal(S, S.T)
            f = ExactFactor(S)
            self.factors[key] = (S, f, f.logdet(), f.kappa())
        return self.factors[key]

    def rows(self, name, spec, arrays):
        self.specs[name] = spec
        for k, v in arrays.items():
            self.arrays["in/%s/%s" % (name, k)] = v
        extra = {k: arrays[k] for k in ("E", "t") if k in arrays}
        return AB.make_inputs(name, spec, arrays["c"], extra.get("E"), extra.get("t"))

    def add(self, name, entry, kind, nu, d, qs, lognorm, inputs, **meta):
        nu32 = float(np.float32(nu)) if kind == "mvt" else 0.0
        lp = [lp_exact(kind, d, nu32, ln, q) for ln, q in zip(lognorm, qs)]
        self.cases.append(dict(name=name, entry=entry, kind=kind, nu=nu32, d=d, inputs=inputs, **meta))
        self.arrays[name + "/lp"] = np.array([float(v) for v in lp])
        self.arrays[name + "/p"] = np.array([round_density(v) for v in lp])
        self.arrays[name + "/q"] = np.array([float(v) for v in qs])
        self.arrays[name + "/lognorm"] = np.array([float(v) for v in lognorm])


def kinds_for(i, d):
    out = [("mvn", 0.0), ("mvt", NUS[i % 7]), ("mvt", NUS[(i + 3) % 7])]
    if d % 2 and ("mvt", 3e7) not in out:
        out.append(("mvt", 3e7))  # float32 nu + d rounds at odd d
    return out


def label(kind, nu):
    return kind if kind == "mvn" else "mvt%g" % nu


def add_pdf(w, d, sname, kinds, far=False):
    S, f, logdet, kap = w.factor(sname, d)
    name = "pdf/%s_d%d%s" % (sname, d, "_far" if far else "")
    if far:
        spec = dict(entry="pdf_batch", d=d, mu="far")
        targets = [d, d, d]
    else:  # mu of the covariance's scale; mu = 0 at d = 64 (the assembly kernel's shape)
        spec = dict(entry="pdf_batch", d=d, mu=0.0 if d == 64 else math.sqrt(S[0, 0]))
        targets = [0, 1e-20, 1e-20, d, d, d, 1e6, 1e6, 1e100]
        ln_mvn = float(lognorm_exact("mvn", d, 0.0, logdet))
        if ln_mvn + 727.0 > 0:  # MVN density exp(-727) (subnormal)
            targets.append(2 * (ln_mvn + 727.0))
    U = AB.uniform(AB.key(name, "U"), (len(targets), d))
    inp = w.rows(name, spec, dict(c=row_scales(S, U, targets)))
    qs = [f.q(residual_centred(x, inp["mu"])) for x in inp["X"]]
    for kind, nu in kinds:
        ln = [lognorm_exact(kind, d, float(np.float32(nu)), logdet)] * len(qs)
        w.add("%s_%s" % (name, label(kind, nu)), "pdf_batch", kind, nu, d, qs, ln, name, sigma=sname,
              kappa2=kap[0], kappa=kap[1])


def add_reweight_identity(w, d, kinds):
    S, f, logdet, kap = w.factor("spd", d)
    name = "reweight_I/d%d" % d
    targets = [0, 1e-20, d, d, 1e6, 1e100]
    U = AB.uniform(AB.key(name, "U"), (len(targets), d))
    inp = w.rows(name, dict(entry="reweight", d=d, F="I"), dict(c=row_scales(S, U, targets)))
    qs = [f.q(residual_centred(x, inp["y"])) for x in inp["X"]]
    for kind, nu in kinds:
        ln = [lognorm_exact(kind, d, float(np.float32(nu)), logdet)] * len(qs)
        w.add("%s_%s" % (name, label(kind, nu)), "reweight", kind, nu, d, qs, ln, name, sigma="spd",
              kappa2=kap[0], kappa=kap[1])


def add_reweight_general(w, d, sname, fkind, kinds):
    """r = y - F x with y and x of unit scale (x = 0, unit, 1e3 and 1e50 times unit): no cancellation between y and
    F x, which no fp64 evaluation of W y - W F x could survive."""
    S, f, logdet, kap = w.factor(sname, d)
    name = "reweight_F/%s_d%d_%s" % (sname, d, fkind)
    inp = w.rows(name, dict(entry="reweight", d=d, F=fkind), dict(c=np.array([0.0, 1.0, 1.0, 1.0, 1e3, 1e50])))
    qs = [f.q(residual_affine(inp["y"], inp["F"], x)) for x in inp["X"]]
    for kind, nu in kinds:
        ln = [lognorm_exact(kind, d, float(np.float32(nu)), logdet)] * len(qs)
        w.add("%s_%s" % (name, label(kind, nu)), "reweight", kind, nu, d, qs, ln, name, sigma=sname,
              kappa2=kap[0], kappa=kap[1])


def add_percov(w, d, n=48):
    """one covariance per particle: graded(E_i) 2^t_i, E_i over 0 .. 33 (kappa ~ 1 .. 1e10), t_i in -13 .. 13"""
    name = "percov/d%d" % d
    E = np.array([round(33 * i / (n - 1)) for i in range(n)], dtype=np.int64)
    t = ((AB.words(AB.key(name, "t"), n) % np.uint64(27)).astype(np.int64) - 13)
    spec = dict(entry="percov", d=d)
    probe = AB.make_inputs(name, spec, np.zeros(n), E, t)  # mu and sigma do not depend on c
    U = AB.uniform(AB.key(name, "U"), (n, d))
    targets = [0.0, 1e-20, 1e6] + [float(d)] * (n - 3)
    c = np.array([row_scales(probe["sigma"][i], U[i:i + 1], [targets[i]])[0] for i in range(n)])
    facs = [ExactFactor(probe["sigma"][i]) for i in range(n)]
    logdets = [fa.logdet() for fa in facs]
    kap = np.array([fa.kappa() for fa in facs])
    inp = w.rows(name, spec, dict(c=c, E=E, t=t, logdet=np.array([float(v) for v in logdets]), kappa=kap[:, 1],
                                  kappa2=kap[:, 0]))
    qs = [fa.q(residual_centred(x, m)) for fa, x, m in zip(facs, inp["X"], inp["mu"])]
    for kind, nu in (("mvn", 0.0), ("mvt", NUS[d % 7])):
        ln = [lognorm_exact(kind, d, float(np.float32(nu)), ld) for ld in logdets]
        w.add("%s_%s" % (name, kind), "percov", kind, nu, d, qs, ln, name)


def add_asm_pool(w):
    d = 64
    S, f, logdet, kap = w.factor("spd", d)
    name = "asm64"
    targets = [0.0, 1e-20, 1e6, 1e100] * 4 + [float(d)] * 240
    targets = [targets[i] for i in np.argsort(AB.uniform(AB.key(name, "order"), len(targets)), kind="stable")]
    U = AB.uniform(AB.key(name, "U"), (len(targets), d))
    inp = w.rows(name, dict(entry="pdf_batch", d=d, mu=0.0), dict(c=row_scales(S, U, targets)))
    qs = [f.q(residual_centred(x, inp["mu"])) for x in inp["X"]]
    ln = [lognorm_exact("mvn", d, 0.0, logdet)] * len(qs)
    w.add("asm64", "pdf_batch", "mvn", 0.0, d, qs, ln, name, sigma="spd", kappa2=kap[0], kappa=kap[1])


def main():
    t0 = time.time()
    w = Writer()
    for i, d in enumerate(DIMS):
        add_pdf(w, d, "spd", kinds_for(i, d))
        add_pdf(w, d, "spd", [("mvn", 0.0), ("mvt", 4.0)], far=True)
        print("d = %d: %.0f s" % (d, time.time() - t0), file=sys.stderr)
    for d in HARD_DIMS:
        for sname in ("g4", "g8", "g12", "dcd", "sm30", "sp30"):
            add_pdf(w, d, sname, [("mvn", 0.0), ("mvt", 4.0), ("mvt", 0.5)])
        print("hard d = %d: %.0f s" % (d, time.time() - t0), file=sys.stderr)
    for d in (3, 17, 64, 200, 320):
        add_reweight_identity(w, d, [("mvn", 0.0), ("mvt", 2.5)])
    for d in (8, 17, 64, 200, 320):
        add_reweight_general(w, d, "spd", "mild", [("mvn", 0.0), ("mvt", 4.0)])
    for d in (8, 64, 200):
        add_reweight_general(w, d, "spd", "hard", [("mvn", 0.0), ("mvt", 4.0)])
        add_reweight_general(w, d, "g8", "mild", [("mvn", 0.0)])
    for d in range(1, 17):
        add_percov(w, d)
    add_asm_pool(w)
    w.arrays["meta"] = np.array(json.dumps(dict(cases=w.cases, inputs=w.specs), sort_keys=True))
    with open(OUT, "wb") as fh:
        np.savez_compressed(fh, **{k: w.arrays[k] for k in sorted(w.arrays)})
    print("%d cases, %.0f kB, %.0f s" % (len(w.cases), os.path.getsize(OUT) / 1024, time.time() - t0),
          file=sys.stderr)


if __name__ == "__main__":
    main()
