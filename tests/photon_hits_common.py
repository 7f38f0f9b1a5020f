"""Shared by tests/test_photon_hits.py, tests/test_photon_hits_gpu.py and tests/test_photon_hits_adapter.py: an independent numpy
restatement of the photon hits definition (include/clsimhip.h, "Photon hits") -- the efficiency rule, the series search as the
bisection it is defined as, the per-record steps in binary64, np.lexsort for the order -- and the inputs the tests use, all made from
committed material: the golden photon records and tests/frame_photons_common.py's synthetic ones, run through the frame photons
stage's host twin."""
import functools

import numpy as np

from clsim_amd import _lib
from clsim_amd import converter as CV
from clsim_amd.tabulator import I3CLSimFunctionPolynomial
from oracle import capi
from tests import frame_photons_common as F
from tests import mcpe_common as M

U64 = np.uint64
SEED = 20240607
NAN = float("nan")
CANONICAL_NAN = np.uint64(0x7ff8000000000000).view(np.float64)


# ---- the maker's description: what both the library and the restatement are made from ----
def spec(doms, tables=None, coefficients=None, oversize=M.OVERSIZE, pancake=M.OVERSIZE, default=NAN, replace=False, ignore_inactive=False,
         only_warn=False, seed=SEED, dom_radius=M.DOM_RADIUS):
    """tables: one (start, step, values) or one constant per class"""
    return dict(doms=np.ascontiguousarray(doms, dtype=CV.PHOTON_HIT_DOM_DTYPE), tables=[M.acceptance_table()] if tables is None else tables,
                coefficients=M.angular_coefficients() if coefficients is None else np.asarray(coefficients, dtype=np.float64), oversize=oversize,
                pancake=pancake, default=default, replace=replace, ignore_inactive=ignore_inactive, only_warn=only_warn, seed=seed, dom_radius=dom_radius)


def maker_of(s):
    funcs = [CV.I3CLSimFunctionConstant(t) if np.isscalar(t) else CV.I3CLSimFunctionFromTable(t[0], t[1], t[2]) for t in s["tables"]]
    return CV.PhotonHitMaker(funcs, I3CLSimFunctionPolynomial(s["coefficients"]), s["doms"], DOMRadiusWithoutOversize=s["dom_radius"],
                             DOMOversizeFactor=s["oversize"], DOMPancakeFactor=s["pancake"], DefaultRelativeDOMEfficiency=s["default"],
                             ReplaceRelativeDOMEfficiencyWithDefault=s["replace"], IgnoreDOMsWithoutDetectorStatusEntry=s["ignore_inactive"],
                             OnlyWarnAboutInvalidPhotonPositions=s["only_warn"], seed=s["seed"])


def dom_table(strings, oms, efficiencies=(1.0,), spe=NAN, two_classes=False, rotated=False, inactive_every=0, out_of_calibration_every=0):
    """one entry per (string, OM): efficiencies dealt round robin, class by string parity, direction (0, 0, -1) -- with which the
    cosine is the MCPE generator's -dir.z -- or (1, 2, 3) / sqrt(14) on odd strings"""
    strings, oms = np.asarray(strings, dtype=np.int32), np.asarray(oms, dtype=np.uint32)
    d = np.zeros(len(strings), dtype=CV.PHOTON_HIT_DOM_DTYPE)
    d["stringID"], d["omID"] = strings, oms
    d["flags"] = CV.PHOTON_HIT_HAS_STATUS | CV.PHOTON_HIT_IN_CALIBRATION
    index = np.arange(len(d))
    if inactive_every:
        d["flags"][index % inactive_every == 3] &= ~np.uint32(CV.PHOTON_HIT_HAS_STATUS)
    if out_of_calibration_every:
        d["flags"][index % out_of_calibration_every == 1] &= ~np.uint32(CV.PHOTON_HIT_IN_CALIBRATION)
    d["relativeDOMEff"] = np.asarray(efficiencies, dtype=np.float64)[index % len(efficiencies)]
    d["speCompensationFactor"] = spe
    d["classIndex"] = (strings & 1) if two_classes else 0
    d["dir"] = (0.0, 0.0, -1.0)
    if rotated:
        d["dir"][(strings & 1) == 1] = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    return d


def resolve_efficiency(s):
    """the reference's rule (I3PhotonToMCPEConverter.cxx:327-388) per DOM; raises ValueError where it log_fatals"""
    d, default = s["doms"], s["default"]
    if default < 0:
        raise ValueError("default < 0")
    out = np.zeros(len(d))
    for i in range(len(d)):
        eff, factor = d["relativeDOMEff"][i], d["speCompensationFactor"][i]
        if s["replace"] or not (d["flags"][i] & CV.PHOTON_HIT_IN_CALIBRATION) or np.isnan(eff):
            if np.isnan(default):
                raise ValueError("no default for DOM %d" % i)
            out[i] = default
        else:
            out[i] = eff * (1.0 if np.isnan(factor) else factor)
    return out


def series_of(first, n):
    """for i = 0 ... n - 1: the bisection of the definition -- the last entry with first <= i, -1 for none -- whatever `first` holds"""
    i = np.arange(n, dtype=np.int64)
    first = np.asarray(first, dtype=np.int64)
    lo, hi = np.zeros(n, dtype=np.int64), np.full(n, len(first), dtype=np.int64)
    while (lo < hi).any():
        active = lo < hi
        mid = lo + (hi - lo) // 2
        goes_right = active & (first[np.minimum(mid, len(first) - 1)] <= i)
        lo = np.where(goes_right, mid + 1, lo)
        hi = np.where(active & ~goes_right, mid, hi)
    return lo - 1


def acceptance(tables, k, wlen):
    A = np.zeros(len(wlen))
    for index, table in enumerate(tables):
        if np.isscalar(table):
            A = np.where(k == index, float(table), A)
            continue
        start, step, values = table[0], table[1], np.asarray(table[2], dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            q = (wlen - start) / step
            fbin = np.trunc(q)
            frac = q - fbin
        low = (fbin < 0) | ((fbin == 0) & (frac < 0))
        high = ~low & ~(fbin < len(values) - 1)
        fbin = np.where(low, 0.0, np.where(high, len(values) - 2.0, fbin))
        frac = np.where(low, 0.0, np.where(high, 1.0, frac))
        b = fbin.astype(np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            a = values[b] + (values[b + 1] - values[b]) * frac
        A = np.where(k == index, a, A)
    return A


def numpy_hits(records, series, s):
    """(mcpes, series, counters) of the definition"""
    r = np.ascontiguousarray(records, dtype=CV.FRAME_PHOTON_DTYPE)
    t = np.ascontiguousarray(series, dtype=CV.MCPE_SERIES_DTYPE)
    n = len(r)
    counters = dict.fromkeys(CV.PHOTON_HIT_COUNTERS, 0)
    efficiency = resolve_efficiency(s)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        owner = series_of(t["first"], n) if len(t) else np.full(n, -1, dtype=np.int64)
        at = np.maximum(owner, 0)
        i = np.arange(n, dtype=np.int64)
        entry = t[at] if len(t) else np.zeros(n, dtype=CV.MCPE_SERIES_DTYPE)
        uncovered = (owner < 0) | (i - entry["first"].astype(np.int64) >= entry["count"].astype(np.int64))
        counters["uncovered"] = int(uncovered.sum())
        alive = ~uncovered
        mismatch = (r["stringID"] != entry["stringID"]) | (r["omID"] != entry["omID"])
        counters["series_mismatch"] = int((alive & mismatch).sum())
        alive &= ~mismatch
        codes = F.dom_code(s["doms"]["stringID"], s["doms"]["omID"])
        order = np.argsort(codes)
        code = F.dom_code(entry["stringID"], entry["omID"])
        where = np.minimum(np.searchsorted(codes[order], code), max(len(codes) - 1, 0))
        dom = order[where] if len(codes) else np.zeros(n, dtype=np.int64)
        known = (codes[dom] == code) if len(codes) else np.zeros(n, dtype=bool)
        counters["unknown_dom"] = int((alive & ~known).sum())
        alive &= known
        d = s["doms"][dom] if len(codes) else np.zeros(n, dtype=CV.PHOTON_HIT_DOM_DTYPE)
        if s["ignore_inactive"]:
            inactive = (d["flags"] & CV.PHOTON_HIT_HAS_STATUS) == 0
            counters["inactive"] = int((alive & inactive).sum())
            alive &= ~inactive
        W = r["weight"].astype(np.float64)
        counters["negative_weight"] = int((alive & (W < 0.0)).sum())
        alive &= ~(W < 0.0)
        alive &= ~(W == 0.0)
        st, ct = capi.eval_math(2, r["theta"]).astype(np.float64), capi.eval_math(3, r["theta"]).astype(np.float64)
        sp, cp = capi.eval_math(2, r["phi"]).astype(np.float64), capi.eval_math(3, r["phi"]).astype(np.float64)
        dx, dy, dz = st * cp, st * sp, ct
        D = d["dir"]
        c = -(dx * D[:, 0] + dy * D[:, 1] + dz * D[:, 2])
        c = np.where(c < 1.0, c, 1.0)
        c = np.where(c > -1.0, c, -1.0)
        x, y, z = (r[k].astype(np.float64) for k in ("x", "y", "z"))
        if s["pancake"] == 1.0:
            R = s["oversize"] * s["dom_radius"]
            lo, hi = max(R - 0.03, 0.0), R + 0.03
            r2 = x * x + y * y + z * z
            off = ~((lo * lo <= r2) & (r2 <= hi * hi))
            counters["off_surface"] = int((alive & off).sum())
            if not s["only_warn"]:
                alive &= ~off
        P = W * acceptance(s["tables"], d["classIndex"], r["wavelength"].astype(np.float64))
        coefficients = s["coefficients"]
        total = np.full(n, coefficients[0])
        multiplier = np.ones(n)
        for coefficient in coefficients[1:]:
            multiplier = multiplier * c
            total = total + coefficient * multiplier
        P = P * total
        P = P * (efficiency[dom] if len(codes) else np.zeros(n))
        above = P > 1.0
        counters["probability_above_one"] = int((alive & above).sum())
        alive &= ~above
        words = r.view(U64).reshape(n, 6)
        h = np.full(n, s["seed"], dtype=U64)
        for j in range(6):
            h = M._splitmix64(h ^ words[:, j])
        u = (h >> U64(11)).astype(np.float64) * 2.0 ** -53
        alive &= ~(P <= u)
        dot = (-x) * dx + (-y) * dy + (-z) * dz
        time = r["time"] + dot * (1.0 - s["pancake"] / s["oversize"]) / r["groupVelocity"].astype(np.float64)
        time = np.where(np.isnan(time), CANONICAL_NAN, time)
    kept = np.flatnonzero(alive)
    kept = kept[np.lexsort((r["id"][kept], F.tkey_of(time[kept]), owner[kept]))]
    out = np.zeros(len(kept), dtype=CV.MCPE_DTYPE)
    out["id"], out["stringID"], out["omID"], out["time"] = r["id"][kept], entry["stringID"][kept], entry["omID"][kept], time[kept]
    group = owner[kept]
    head = np.ones(len(kept), dtype=bool)
    head[1:] = group[1:] != group[:-1]
    first = np.flatnonzero(head)
    out_series = np.zeros(len(first), dtype=CV.MCPE_SERIES_DTYPE)
    source = t[group[first]] if len(first) else t[:0]
    out_series["frame"], out_series["stringID"], out_series["omID"], out_series["first"] = source["frame"], source["stringID"], source["omID"], first
    out_series["count"] = np.diff(np.append(first, len(kept)))
    return out, out_series, counters


def same(got, want):
    for g, w in zip(got[:2], want[:2]):
        assert g.dtype == w.dtype and len(g) == len(w) and g.tobytes() == w.tobytes()
    assert got[2] == want[2]


def write_input(path, records, series, s):
    """the maker's description and the input as tests/photon_hits_host_main.cpp and clsim_amd/cxx/photon_hits_adapter_test.cxx read them"""
    sizes = [0 if np.isscalar(t) else len(t[2]) for t in s["tables"]]
    assert all(float(t) == 1.0 for t in s["tables"] if np.isscalar(t))
    cfg = _lib.PhotonHitConfig(s["dom_radius"], s["oversize"], s["pancake"], s["default"], int(s["replace"]), int(s["ignore_inactive"]),
                               int(s["only_warn"]), 0, s["seed"])
    with open(path, "wb") as f:
        f.write(np.array([len(sizes), len(s["coefficients"]), len(s["doms"]), len(records), len(series)] + sizes, dtype=np.uint64).tobytes())
        for t in s["tables"]:
            if not np.isscalar(t):
                f.write(np.array([t[0], t[1]], dtype=np.float64).tobytes() + np.asarray(t[2], dtype=np.float64).tobytes())
        f.write(np.asarray(s["coefficients"], dtype=np.float64).tobytes() + bytes(cfg) + s["doms"].tobytes())
        f.write(np.ascontiguousarray(records, dtype=CV.FRAME_PHOTON_DTYPE).tobytes() + np.ascontiguousarray(series, dtype=CV.MCPE_SERIES_DTYPE).tobytes())


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def fixture_records(name):
    """the golden photon records of `name` as frame photons: a particle table of three frames, no mask"""
    photons = M.fixture_photons(name)
    strings, oms = M.all_pairs()
    records, series, counters = CV.FramePhotonDoms(strings, oms).MakeFramePhotonsHost(photons, F.particle_table(photons["id"]))
    assert len(records) == len(photons) and not any(counters.values()) and len(set(series["frame"])) == 3
    return records, series


@functools.lru_cache(maxsize=None)
def synthetic_records(n, seed, special=True, quantised=True):
    """frame_photons_common.synthetic_photons as frame photons: quantised times, so many equal and near-equal times per series.
    Positions are put on the DOM's oversized sphere but for every ninth record."""
    photons = F.synthetic_photons(n, seed, special=special, quantised=quantised)
    rng = np.random.default_rng(seed + 1000)
    direction = rng.standard_normal((n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    radius = np.where(np.arange(n) % 9 == 4, 1.0, M.OVERSIZE * M.DOM_RADIUS + rng.uniform(-0.02, 0.02, n))
    for k, name in enumerate(("x", "y", "z")):
        photons[name] = direction[:, k] * radius
    photons["weight"][np.arange(n) % 50 == 7] = 0.0
    records, series, counters = F.synthetic_doms().MakeFramePhotonsHost(photons, F.particle_table(photons["id"]))
    assert len(records) == n and not any(counters.values())
    return records, series


def adversarial_records(n, seed):
    """synthetic records with NaNs, infinities, denormals, huge angles and zeros in every float field, NaN times and zero group
    velocities, a few hundred of each"""
    records, series = synthetic_records(n, seed)
    records = records.copy()
    rng = np.random.default_rng(seed + 7)
    specials = np.array([np.nan, np.inf, -np.inf, 1e-45, -1e-45, 3e38, -3e38, 0.0, -0.0, 4e9, -4e9, 1e20], dtype=np.float32)
    for name in F.FLOATS:
        at = rng.choice(n, n // 20, replace=False)
        records[name][at] = specials[rng.integers(0, len(specials), len(at))]
    at = rng.choice(n, n // 40, replace=False)
    records["time"][at] = np.array([np.nan, np.inf, -np.inf, -0.0, 5e-324, 1e300])[rng.integers(0, 6, len(at))]
    negative_nan = rng.choice(n, 8, replace=False)
    records["time"].view(U64)[negative_nan] = 0xFFF8000000000001
    records["groupVelocity"][rng.choice(n, n // 40, replace=False)] = 0.0
    return records, series


def keep_all(strings, oms, **kwargs):
    """a maker under which a record of weight 1 has P = 1 exactly and is kept whatever the draw: constant acceptance 1, polynomial 1,
    efficiency 1"""
    return spec(dom_table(strings, oms), tables=[1.0], coefficients=[1.0], **kwargs)


CONFIGURATIONS = ("check_off", "correction_live", "two_classes", "rotated", "efficiencies", "inactive", "warn_on", "warn_off", "check_on")


def configuration(name, strings, oms):
    """the CPU list of configurations over a DOM list"""
    scaled = [M.acceptance_table(), M.acceptance_table(0.5)]
    if name == "check_off":             # pancake = oversize: no check, no correction
        return spec(dom_table(strings, oms))
    if name == "check_on":              # pancake 1: the check, against oversize x R
        return spec(dom_table(strings, oms), pancake=1.0)
    if name == "correction_live":
        return spec(dom_table(strings, oms), pancake=2.0)
    if name == "two_classes":
        return spec(dom_table(strings, oms, two_classes=True), tables=scaled)
    if name == "rotated":
        return spec(dom_table(strings, oms, two_classes=True, rotated=True), tables=scaled, pancake=2.0)
    if name == "efficiencies":
        return spec(dom_table(strings, oms, efficiencies=(0.5, 1.0, 1.35), spe=1.0, out_of_calibration_every=7), default=0.9)
    if name == "inactive":
        return spec(dom_table(strings, oms, inactive_every=10), ignore_inactive=True)
    if name == "warn_on":
        return spec(dom_table(strings, oms), pancake=1.0, only_warn=True)
    if name == "warn_off":
        return spec(dom_table(strings, oms, efficiencies=(0.5, 1.0)), pancake=1.0, only_warn=False)
    raise KeyError(name)
