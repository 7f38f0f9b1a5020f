"""Float64 numpy statements of the photon loop's SAMPLERS -- the uniform draw, the scattering-angle cosine and the wavelength generators
-- written from the reference's HOST classes (random_value/I3CLSimRandomValueHenyeyGreenstein.cxx, ...SimplifiedLiu.cxx, ...
MixedDistribution.cxx, ...InterpolatedDistribution.cxx, ...WlenCherenkovNoDispersion.cxx, ...Constant.cxx).  Nothing here shares code
or expression order with oracle/ or clsim_amd/csrc/.  tests/test_sampler_reference.py holds the oracle to these statements draw by
draw, tests/test_sampler_reference_gpu.py the tester kernel; tests/sampler_common.py makes the draws.

A draw is a 32 bit WORD of the generator.  u = 2^-24 is the unit roundoff of binary32 (tests/propagation_reference.py, whose U, SAFETY
and ulp32 are used); the tests assert SAFETY times the first order bounds below and hold the oracle to the bounds themselves.

(1) THE UNIFORM (mwcrng_kernel.cl:12-28).  rand_co = convert_float_rtz(word) / 2^32: the word truncated to its 24 leading significant
    bits, over 2^32 -- exact, no tolerance.  rand_oc = 1 - rand_co in binary32, the difference rounded to nearest: r = 1 exactly for
    every word below 2^7, and r > 0 always.

(2) THE SCATTERING COSINE.  f (the SimplifiedLiu fraction) and g (the mean cosine) are the binary32 values the tables hold.
    Mixed.cxx, single random number form: U < f -> SimplifiedLiu with v = U / f, otherwise HenyeyGreenstein with v = (1 - U) / (1 - f).
      HG (HenyeyGreenstein.cxx:69-92): s = 2 v - 1, c = (1 + g^2 - ((1 - g^2) / (1 + g s))^2) / (2 g)
      Liu (SimplifiedLiu.cxx:64-88):   c = 2 v^beta - 1, beta = (1 - g) / (1 + g)
    both clipped to [-1, 1].  The roundings of the reference's device expression, first order:
      v:    pure forms: exact.  Mixed, Liu: one division, dv = u v.  Mixed, HG: 1 - U is exact in binary32; the divisor is the literal
            of the DOUBLE 1 - f_double, off 1 - f by u f + u (1 - f) = u; the division u: dv = u v (1 + 1 / (1 - f)).
      HG:   ds = 2 dv + u |s|.  den = 1 + g s: d den = g ds + u g |s| + u den.  The literal g^2 is that of the double g squared, off
            g^2 by 3 u g^2 (g itself by u g, twice; the literal's own rounding): num = 1 - g^2 moves by 3 u g^2 + u num, 1 + g^2 by
            3 u g^2 + u (1 + g^2).  q = num / den: relative dnum / num + dden / den + u; q^2 twice that + u; the difference with
            1 + g^2 adds u |difference|; the division by 2 g (exact doubling) u |c|.
            => dc = (3 u g^2 + u (1 + g^2) + q^2 (2 (dnum / num + dden / den + u) + u) + u |1 + g^2 - q^2|) / (2 g) + u |c|
            Towards s = -1 (v -> 0, backward scattering: c -> -1) den = 1 - g = 0.1 amplifies the rounding of s tenfold and q^2 = (1 + g)^2 is
            3.6: this is the largest term, about 140 u for g = 0.9.
      Liu:  the literal beta is that of the double (1 - g_d) / (1 + g_d): relative u g / (1 - g) + u g / (1 + g) + u =: r_beta (10 u for
            g = 0.9: THE LARGEST TERM, 2 v^beta |ln v| beta r_beta <= 2 r_beta / e = 7.7 u).  powr is good to 1.3 ulp on (1e-9, 1]
            (tests/test_oracle.py), taken as 2 ulp = 4 u.  p = v^beta: dp = p (beta dv / v + beta |ln v| r_beta + 4 u);
            dc = 2 dp + u |c|.
    Clipping moves a value towards the true one, which lies in [-1, 1].
    The analytic CDFs (for the Kolmogorov distance): Liu ((c + 1) / 2)^(1 / beta); HG (1 - g^2) / (2 g) (1 / sqrt(1 + g^2 - 2 g c) -
    1 / (1 + g)); the mixture f Liu + (1 - f) HG.

(3) THE INTERPOLATED DISTRIBUTION (InterpolatedDistribution.cxx:137-175 InitTables, :236-336 the generated function; constant spacing
    or its own abscissae).  The density is piecewise linear through (x_j, y_j); F is its exact piecewise quadratic CDF, normalised, in
    float64; beta_j = y_j / total, m_k the probability of bin k, acu_k = F(x_k).  A draw (r, w) is held FORWARD: |F(w) - r| <= bound.
    The inverse is ill-conditioned exactly where a density falls to zero (dF/dw -> 0), the forward form is not.  The reference takes the
    first bin k with acu32[k + 1] >= r and returns x0 + t, t the root of G(t) = b t + slope t^2 / 2 = dy, dy = r - acu32[k], written
    t = q (sqrt(D) - 1) with q = b / slope, D = 1 + 2 dy / (b q).  G = b q (D - 1) / 2 is LINEAR in D and G = b q (S^2 - 1) / 2 in S =
    sqrt(D), so errors of D and S pass into F without the 1 / sqrt(D) of the inverse.
      (a) the cumulative table: accumulated in DOUBLE on the host (InitTables) and written as a literal -- one rounding per entry,
          u acu_k, however many entries there are (nothing accumulates in single precision).
      (b) dy: one subtraction, u m_k.  The literals b and beta_(k+1) (u each), their difference, the spacing and the division in the
          slope: G moves by u b t + (u (b + b') + 3 u |b' - b|) t^2 / (2 sp) <= 6 u m_k.
      (c) the root: e = dy (2 slope) / (b b) carries four roundings, D = e + 1 one: dD = 4 u |e| + u D, which G takes as
          b |q| dD / 2 = 4 u dy + u b |q| D / 2.  The square root: dS = u S, G takes b |q| S dS = u b |q| D.  Then (S - 1), times b,
          over slope: 3 u relative in t, G takes density t 3 u <= 6 u m_k.  With b |q| D <= b |q| + 2 dy:
          (4 + 3 + 6) u m_k + 1.5 u b |q|, and b |q| = beta_k^2 sp / |beta_(k+1) - beta_k| =: C_k, THE CONDITIONING of sqrt(D) - 1 in a
          nearly flat bin (D -> 1).  A bin that is exactly flat takes the branch dy / b (no C_k).  The whole term 1.5 u C_k is capped
          at m_k: the result stays in its bin (asserted separately), where F moves by m_k at most.
      (d) the abscissa: x0 = k spacing + first with both literals, a product and a sum -- 3 u x; the final sum u x: dx = 4 u x (its own
          abscissae: the literal and the final sum, 2 u x).  F takes max(beta_k, beta_(k+1)) dx.
      => bound_k = u (acu_(k+1) + 20 m_k) + min(1.5 u C_k, m_k) + max(beta_k, beta_(k+1)) dx
    WHICH TERM DOMINATES: (d), the rounding of the abscissa itself times the density.  A wavelength of 4e-7 m is known to 2.4e-14 m;
    an LED's spectrum is ~2e-8 m wide, so that is 1e-6 of the distribution -- ten times the whole of (a) ... (c).  Where the
    Cherenkov spectrum times the acceptance peaks (nearly flat bins) (c)'s C_k comes second.
    A result within dx of a node is judged with the larger bound of the two bins.
    WHERE THE DRAW LANDS: between the nodes x_k and x_(k'+1) of the first and the last bin whose [acu_k, acu_(k+1)] holds r up to the
    tables' rounding (u), up to dx.

(4) WlenCherenkovNoDispersion.cxx:72-92: w = 1 / (1 / to + r (1 / from - 1 / to)): two literals, a product, a sum, a division: 5 u w.
    RandomValueConstant: the literal, u |value|; no draw is used.
"""
import numpy as np

from tests.propagation_reference import U, SAFETY, ulp32          # noqa: F401  (re-exported for the tests)


# ---------------------------------------------------------------------------------------------------------------------------------
# (1) the uniform
# ---------------------------------------------------------------------------------------------------------------------------------

def uniform_co(words):
    """[0, 1): the word truncated to 24 significant bits, over 2^32 (exact in float64)"""
    w = np.asarray(words, dtype=np.uint64)
    _, e = np.frexp(w.astype(np.float64))                  # e = bit length (0 for the word 0)
    drop = np.maximum(e.astype(np.int64) - 24, 0).astype(np.uint64)
    return ((w >> drop) << drop).astype(np.float64) / 4294967296.0


def uniform_oc(words):
    """(0, 1]: 1 - u, rounded to binary32 (1 - u is exact in float64, the cast rounds to nearest even as the subtraction does)"""
    return (1.0 - uniform_co(words)).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# (2) the scattering cosine
# ---------------------------------------------------------------------------------------------------------------------------------

def liu_beta(g):
    return (1.0 - g) / (1.0 + g)


def hg_cos(v, dv, g):
    """(c, dc) of HenyeyGreenstein for v known to dv"""
    s = 2.0 * v - 1.0
    ds = 2.0 * dv + U * np.abs(s)
    den = 1.0 + g * s
    dden = g * ds + U * g * np.abs(s) + U * den
    num = 1.0 - g * g
    dnum = 3.0 * U * g * g + U * num
    q2 = (num / den) ** 2
    dq2 = q2 * (2.0 * (dnum / num + dden / den + U) + U)
    top = 1.0 + g * g - q2
    dtop = 3.0 * U * g * g + U * (1.0 + g * g) + dq2 + U * np.abs(top)
    c = top / (2.0 * g)
    return np.clip(c, -1.0, 1.0), dtop / (2.0 * g) + U * np.abs(c)


def liu_cos(v, dv, g):
    """(c, dc) of SimplifiedLiu for v known to dv"""
    beta = liu_beta(g)
    r_beta = U * g / (1.0 - g) + U * g / (1.0 + g) + U
    safe = np.maximum(v, 1e-300)
    p = np.where(v > 0.0, safe ** beta, 0.0)
    dp = np.where(v > 0.0, p * (beta * dv / safe + beta * np.abs(np.log(safe)) * r_beta + 4.0 * U), 0.0)
    c = 2.0 * p - 1.0
    return np.clip(c, -1.0, 1.0), 2.0 * dp + U * np.abs(c)


def scattering_cos(words, kind, g, f=None):
    """kind: 'hg', 'liu' or 'mixed' (f: the SimplifiedLiu fraction).  Returns (c, bound, is_liu)."""
    u = uniform_co(words)
    g = float(g)
    if kind == "hg":
        c, dc = hg_cos(u, np.zeros_like(u), g)
        return c, dc, np.zeros(u.shape, bool)
    if kind == "liu":
        c, dc = liu_cos(u, np.zeros_like(u), g)
        return c, dc, np.ones(u.shape, bool)
    assert kind == "mixed"
    f = float(f)
    is_liu = u < f
    v_l = u / f
    c_l, d_l = liu_cos(v_l, U * v_l, g)
    v_h = (1.0 - u) / (1.0 - f)
    c_h, d_h = hg_cos(v_h, U * v_h * (1.0 + 1.0 / (1.0 - f)), g)
    return np.where(is_liu, c_l, c_h), np.where(is_liu, d_l, d_h), is_liu


def liu_cdf(c, g):
    return ((np.asarray(c, dtype=np.float64) + 1.0) / 2.0) ** (1.0 / liu_beta(g))


def hg_cdf(c, g):
    c = np.asarray(c, dtype=np.float64)
    return (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * c) - 1.0 / (1.0 + g))


def scattering_cdf(c, kind, g, f=None):
    g = float(g)
    if kind == "hg":
        return hg_cdf(c, g)
    if kind == "liu":
        return liu_cdf(c, g)
    return float(f) * liu_cdf(c, g) + (1.0 - float(f)) * hg_cdf(c, g)


def kolmogorov_distance(sample, cdf):
    """sup |empirical - cdf| over a sample (both one-sided distances, ties included)"""
    s = np.sort(np.asarray(sample, dtype=np.float64).ravel())
    F = cdf(s)
    n = len(s)
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(0, n) / n)))


KS_1_PERCENT = 1.63                # sup distance sqrt(n) at the 1 % level


# ---------------------------------------------------------------------------------------------------------------------------------
# (3), (4) the wavelength generators
# ---------------------------------------------------------------------------------------------------------------------------------

class Interpolated:
    """the exact CDF of a piecewise linear density through (x_j, y_j), and the bounds of (3)"""

    def __init__(self, y, x=None, first=None, spacing=None):
        self.y = np.asarray(y, dtype=np.float64)
        self.own_x = x is not None
        self.x = np.asarray(x, dtype=np.float64) if self.own_x else float(first) + float(spacing) * np.arange(len(self.y))
        sp = np.diff(self.x)
        mass = sp * (self.y[1:] + self.y[:-1]) / 2.0
        total = mass.sum()
        self.beta = self.y / total
        self.m = mass / total
        self.acu = np.concatenate([[0.0], np.cumsum(mass)]) / total
        self.acu[-1] = 1.0
        self.sp = sp
        b, b1 = self.beta[:-1], self.beta[1:]
        with np.errstate(divide="ignore", invalid="ignore"):
            cond = np.where(b1 != b, b * b * sp / np.abs(b1 - b), 0.0)
        self.cond = np.minimum(1.5 * U * cond, self.m)
        self.dx_rel = (2.0 if self.own_x else 4.0) * U
        self.bin_bound = U * (self.acu[1:] + 20.0 * self.m) + self.cond + np.maximum(b, b1) * self.dx_rel * np.abs(self.x[1:])

    def cdf(self, w):
        w = np.asarray(w, dtype=np.float64)
        k = np.clip(np.searchsorted(self.x, w, side="right") - 1, 0, len(self.x) - 2)
        t = np.clip(w, self.x[0], self.x[-1]) - self.x[k]
        slope = (self.beta[k + 1] - self.beta[k]) / self.sp[k]
        return self.acu[k] + self.beta[k] * t + 0.5 * slope * t * t

    def forward_bound(self, w):
        """bound_k of the bin w lies in; within dx of a node the larger of the two bins'"""
        w = np.asarray(w, dtype=np.float64)
        n = len(self.x)
        dx = self.dx_rel * np.abs(w)
        k = np.clip(np.searchsorted(self.x, w, side="right") - 1, 0, n - 2)
        k_lo = np.clip(np.searchsorted(self.x, w - dx, side="right") - 1, 0, n - 2)
        k_hi = np.clip(np.searchsorted(self.x, w + dx, side="right") - 1, 0, n - 2)
        return np.maximum(self.bin_bound[k], np.maximum(self.bin_bound[k_lo], self.bin_bound[k_hi]))

    def landing_interval(self, r):
        """(low, high, dx): the nodes between which a draw r lands, and the abscissa's first order rounding"""
        r = np.asarray(r, dtype=np.float64)
        n = len(self.x)
        first = np.clip(np.searchsorted(self.acu[1:] * (1.0 + U), r, side="left"), 0, n - 2)
        last = np.clip(np.searchsorted(self.acu[1:] * (1.0 - U), r, side="left"), 0, n - 2)
        return self.x[first], self.x[last + 1], self.dx_rel * np.abs(self.x[last + 1])


def no_dispersion(r, from_wlen, to_wlen):
    """(w, bound) of WlenCherenkovNoDispersion"""
    lo = 1.0 / float(to_wlen)
    w = 1.0 / (lo + np.asarray(r, dtype=np.float64) * (1.0 / float(from_wlen) - lo))
    return w, 5.0 * U * w
