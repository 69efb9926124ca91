"""The error bound every log-density is held to, and the reader of tests/golden/accuracy.npz.

For each element, with the extended-precision reference lp*, q* and lognorm* of the fixture:

    |lp - lp*| <= C u ( sqrt(d) |lognorm*| + |lp* - lognorm*| + d kappa (1 + s q*) ),    u = 2^-53,
    s = 1/2 (MVN),   s = (nu + d) / (2 (nu + q*)) (Student-t, nu + d in float32 as the library forms it)

kappa is kappa_2 of Sigma scaled to unit diagonal, not kappa_2(Sigma): Cholesky and the triangular solve are
invariant under diagonal scaling up to rounding (van der Sluis), so a D C D covariance with D over 1e-8 .. 1e8 is
as hard as C, and kappa_2(Sigma) ~ 1e32 would make its bound vacuous.  The first two terms cover the rounding of
the normalising constant -- a sum of d logarithms (logdet), whose rounding grows like sqrt(d) times its size --
and of the epilogue's own product -- for Student-t far in the tail (nu + d)/2 log1p(q/nu)
is much larger than s q* --, the third the error of logdet (~ d kappa u) and of q (relative ~ d kappa u, times the
sensitivity s q* of lp to a relative change of q).

Densities (log=False): where p* = exp(lp*) is normal, log(p) is held to the same bound; where it is subnormal or
0, |p - p*| <= one subnormal step + p* times the bound; where p* overflows to inf, p must be inf.

C was fixed on the CPU before any GPU run, by emulating the library's arithmetic (tests/test_accuracy_bound.py):
the host factor of hostla.h through a g++ shim, numpy fp64 for W (x - shift), the epilogue and the per-particle
Cholesky.  Over every fixture case the emulation's worst err / bound is CALIBRATED_WORST at C = 1, and C is eight
times that, rounded up, so that the emulation passes with a worst ratio <= 1/8 -- the headroom is for the
matrix cores' summation order.
"""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "accuracy.npz")

U = 2.0 ** -53
# worst err / bound of the CPU emulation at C = 1 (tests/test_accuracy_bound.py): 2.10, on a Student-t row with
# nu = 3e7, d = 1 (the normalising constant's lgamma terms)
CALIBRATED_WORST = 2.125
C = 8 * CALIBRATED_WORST  # 17
TINY = 2.0 ** -1074


# ---- inputs: rebuilt from recipes, bit for bit on every machine ----------------------------------------------------
# The fixture stores no input matrix.  Random numbers come from SplitMix64 in numpy uint64 arithmetic (wraps the same
# everywhere).  Covariances and F are built from +-1 matrices and powers of two only, so every partial sum of their
# matrix products is exact and no summation order, BLAS kernel or FMA can change a bit; the non-power-of-two
# scalings (D C D, 1e-30 / 1e30) are single elementwise IEEE products.

def key(*parts):
    return int.from_bytes(hashlib.sha256("/".join(map(str, parts)).encode()).digest()[:8], "little")


def words(k, n):
    """n SplitMix64 outputs of the stream k"""
    z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(k)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform(k, shape):
    """uniform in [-1, 1), 53 significant bits (exact)"""
    n = int(np.prod(shape))
    return ((words(k, n) >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0).reshape(shape)


def signs(k, shape):
    n = int(np.prod(shape))
    return np.where(words(k, n) >> np.uint64(63), -1.0, 1.0).reshape(shape)


def graded(M, E):
    """M diag(lambda) M^T 2^-s + 2^-E I with lambda_k = 2^-round(E k / (d-1)) and 2^s >= d: eigenvalues in about
    [2^-E, 5]; E = 0 is M M^T 2^-s + I, the well-conditioned family.  Every partial sum is a multiple of 2^-E below
    d in magnitude: exact for E + log2(d) < 52."""
    d = M.shape[0]
    s = (d - 1).bit_length()
    lam = np.array([2.0 ** -round(E * k / (d - 1)) for k in range(d)]) if d > 1 else np.ones(1)
    return ((M * lam) @ M.T) * 2.0 ** -s + 2.0 ** -E * np.eye(d)


GRADED = {"spd": 0, "g4": 13, "g8": 27, "g12": 40}  # scaled kappa ~ 5, 1e4 .. 1e5, 1e8 .. 1e9, 1e12 .. 1e13
SCALED = {"sm30": 1e-30, "sp30": 1e30}


def make_sigma(name, d):
    if name in GRADED:
        return graded(signs(key("M", d), (d, d)), GRADED[name])
    if name in SCALED:
        return make_sigma("spd", d) * SCALED[name]
    if name == "dcd":  # D C D, D from 2^-27 to 2^28 (~1e-8 .. 3e8) with full mantissas, in a random order
        C = make_sigma("spd", d)
        order = np.argsort(uniform(key("dcd perm", d), d), kind="stable")
        expo = np.array([round(-27 + 54 * i / max(d - 1, 1)) for i in range(d)])[order]
        D = (1.5 + 0.5 * uniform(key("dcd D", d), d)) * 2.0 ** expo
        S = (D[:, None] * C) * D[None, :]
        return np.tril(S) + np.tril(S, -1).T
    raise KeyError(name)


def make_F(kind, d, tag):
    s = (d - 1).bit_length()
    if kind == "mild":  # I + M 2^-(s+1): kappa(F) <~ 10
        return np.eye(d) + signs(key("F", tag), (d, d)) * 2.0 ** -(s + 1)
    # "hard": M1 diag(2^-round(20 k / (d-1))) M2^T 2^-s + 2^-20 I, kappa(F) ~ 1e6
    lam = np.array([2.0 ** -round(20 * k / (d - 1)) for k in range(d)])
    P = (signs(key("F1", tag), (d, d)) * lam) @ signs(key("F2", tag), (d, d)).T
    return P * 2.0 ** -s + 2.0 ** -20 * np.eye(d)


def make_inputs(name, spec, c, E=None, t=None):
    """the inputs of the row set `name`: row j is X_j = base + c_j u_j with u_j uniform in [-1, 1)^d"""
    d, n = spec["d"], len(c)
    U = uniform(key(name, "U"), (n, d))
    out = {}
    if spec["entry"] == "percov":
        scale = np.array([2.0 ** (int(ti) // 2) for ti in t])
        out["mu"] = scale[:, None] * uniform(key(name, "mu"), (n, d))
        out["sigma"] = np.array([graded(signs(key(name, "M", i), (d, d)), int(E[i])) * 2.0 ** int(t[i])
                                 for i in range(n)])
        base = out["mu"]
    elif spec["entry"] == "pdf_batch":
        m = spec["mu"]
        u = uniform(key(name, "mu"), d)
        out["mu"] = 1e8 * (1.5 + 0.5 * u) if m == "far" else m * u
        base = out["mu"]
    else:
        out["y"] = uniform(key(name, "y"), d)
        out["F"] = np.eye(d) if spec["F"] == "I" else make_F(spec["F"], d, name)
        base = out["y"] if spec["F"] == "I" else np.zeros(d)
    out["X"] = base + c[:, None] * U
    return out


class Fixture:
    def __init__(self, path=FIXTURE):
        with np.load(path, allow_pickle=False) as z:
            self.a = {k: z[k] for k in z.files}
        meta = json.loads(str(self.a["meta"]))
        self.cases, self.specs = meta["cases"], meta["inputs"]
        self.by_name = {c["name"]: c for c in self.cases}
        self._inputs = {}

    def sigma(self, case):
        return make_sigma(case["sigma"], case["d"])

    def inputs(self, case):
        name = case["inputs"]
        if name not in self._inputs:
            pre = "in/%s/" % name
            arr = {k[len(pre):]: v for k, v in self.a.items() if k.startswith(pre)}
            out = make_inputs(name, self.specs[name], arr["c"], arr.get("E"), arr.get("t"))
            out.update({k: v for k, v in arr.items() if k in ("logdet", "kappa", "kappa2")})
            self._inputs[name] = out
        return self._inputs[name]

    def ref(self, case):
        pre = case["name"] + "/"
        return {k: self.a[pre + k] for k in ("lp", "p", "q", "lognorm")}

    def select(self, entry=None, pred=None):
        return [c for c in self.cases if (entry is None or c["entry"] == entry) and (pred is None or pred(c))]


def kappa_of(fx, case):
    """per-row kappa (percov: one covariance per row)"""
    if case["entry"] == "percov":
        return fx.a["in/%s/kappa" % case["inputs"]]
    return np.full(len(fx.a[case["name"] + "/lp"]), case["kappa"])


def bound(fx, case, c=None):
    c = C if c is None else c
    ref = fx.ref(case)
    d, q = case["d"], ref["q"]
    if case["kind"] == "mvn":
        s = 0.5
    else:
        npd = float(np.float32(np.float32(case["nu"]) + np.float32(d)))
        s = npd / (2.0 * (case["nu"] + q))
    return c * U * (np.sqrt(d) * np.abs(ref["lognorm"]) + np.abs(ref["lp"] - ref["lognorm"]) +
                    d * kappa_of(fx, case) * (1.0 + s * q))


def ratios(fx, case, got, log=True, c=None):
    """err / bound per element (inf where a value is not finite)."""
    ref = fx.ref(case)
    b = bound(fx, case, c)
    got = np.asarray(got, dtype=np.float64)
    if log:
        r = np.abs(got - ref["lp"]) / b
        return np.where(np.isfinite(got), r, np.inf)
    p = ref["p"]
    normal = (p >= 2.0 ** -1022) & np.isfinite(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(normal, np.abs(np.log(np.where(got > 0, got, TINY)) - ref["lp"]) / b,
                     np.abs(got - p) / (TINY + p * b))
    # p* = inf (lp* > log(DBL_MAX), e.g. a covariance scaled by 1e-30): only inf matches
    r = np.where(np.isinf(p), np.where(got == p, 0.0, np.inf), r)
    return np.where(np.isfinite(got) | np.isinf(p), r, np.inf)


def worst(fx, case, got, log=True, c=None):
    r = ratios(fx, case, got, log, c)
    i = int(np.argmax(r))
    return float(r[i]), i


def check(fx, case, got, log=True, label=""):
    """assert every element within the bound; the message names the case and the worst ratio"""
    w, i = worst(fx, case, got, log)
    ref = fx.ref(case)
    assert w <= 1.0, "%s%s (%s): worst err/bound %.3g at row %d (got %r, want %r, q* %.3g, kappa %.3g)" % (
        case["name"], label, "log" if log else "density", w, i, float(np.asarray(got)[i]),
        float(ref["lp"][i] if log else ref["p"][i]), float(ref["q"][i]), float(kappa_of(fx, case)[i]))
    return w


def family(d, ldx=None, aligned=True):
    """the log-pdf kernel run_logpdf() dispatches (d, ldx) to (cusmc_abi.hip, launch.h)"""
    ldx = d if ldx is None else ldx
    if d < 16:
        return "small"
    if d <= 176:
        return "matrix-core" if d % 16 == 0 and ldx % 2 == 0 and aligned else "matrix-core padded"
    if d <= 256:
        return "wide"
    return "generic"
