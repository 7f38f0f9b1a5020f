"""Shared by tests/test_mcpe.py and tests/test_mcpe_gpu.py: the fixtures of the MCPE generator and an independent numpy
restatement of its definition (include/clsimhip.h, "MCPE generator")."""
import json
import os

import numpy as np

from clsim_amd import converter as CV
from clsim_amd.synthetic import PHOTON_DTYPE
from clsim_amd.tabulator import I3CLSimFunctionPolynomial
from oracle import capi

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("mie", "lea", "mie_60_keep", "flasher_led405", "lea_no_pancake", "c1")
SEED = 12345
DOM_RADIUS, OVERSIZE = 0.1651, 5.0
MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def pancake_of(name):
    return 1.0 if name == "lea_no_pancake" else 5.0


def fixture_photons(name):
    """the committed photon records of verbatim_cl_<name>.npz; word 11 holds string and DOM INDICES (0..85, 0..59), which the
    stand-alone tests use as the IDs"""
    fx = np.load(os.path.join(G, "verbatim_cl_%s.npz" % name))
    return np.ascontiguousarray(fx["hits"]).view(PHOTON_DTYPE).reshape(-1).copy()


def acceptance_table(scale=1.0):
    fx = json.load(open(os.path.join(G, "dom_acceptance.json")))
    start, step, values = fx["args"][0], fx["args"][1], np.asarray(fx["args"][2]["ndarray"], dtype=np.float64)
    return start, step, values * scale


def angular_coefficients():
    values = json.load(open(os.path.join(G, "angular_sensitivity_holeice.json")))["values"]
    assert len(values) == 12
    return np.asarray(values[1:], dtype=np.float64)       # the first number is the maximum


def all_pairs():
    s, d = np.meshgrid(np.arange(86), np.arange(60), indexing="ij")
    return s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)


def make_generator(tables, string_ids, om_ids, class_index, pancake=5.0, seed=SEED, coefficients=None):
    """tables: list of (start, step, values)"""
    funcs = [CV.I3CLSimFunctionFromTable(t[0], t[1], t[2]) for t in tables]
    poly = I3CLSimFunctionPolynomial(angular_coefficients() if coefficients is None else coefficients)
    return CV.MCPEGenerator(funcs, string_ids, om_ids, class_index, poly, domRadius=DOM_RADIUS, oversizeFactor=OVERSIZE,
                            pancakeFactor=pancake, seed=seed)


def standard_generator(pancake=5.0, seed=SEED):
    s, d = all_pairs()
    return make_generator([acceptance_table()], s, d, np.zeros(len(s), dtype=np.int32), pancake=pancake, seed=seed)


def _splitmix64(state):
    z = (state + np.uint64(0x9E3779B97F4A7C15)) & MASK
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & MASK
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & MASK
    return z ^ (z >> np.uint64(31))


def numpy_mcpes(photons, tables, class_of, coefficients, pancake, seed=SEED, dom_radius=DOM_RADIUS, oversize=OVERSIZE):
    """The definition once more, in numpy binary64 (the two sin / cos pairs come from the oracle's C restatement of the device math
    library).  tables: list of (start, step, values); class_of(string_ids, om_ids) -> class index per record, -1 = none.
    Returns (mcpes in input order, counters dict, P of the records that reached the draw, accepted mask of those)."""
    ph = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
    w = ph.view(np.uint32).reshape(len(ph), 20)
    W = ph["weight"].astype(np.float64)
    counters = dict.fromkeys(CV.MCPE_CONDITIONS, 0)
    alive = np.ones(len(ph), dtype=bool)
    negative = W < 0.0
    counters["negative_weight"] = int(negative.sum())
    alive &= ~negative
    alive &= ~(W == 0.0)
    x, y, z = (ph[k].astype(np.float64) for k in ("x", "y", "z"))
    r2 = x * x + y * y + z * z
    R = dom_radius * oversize / pancake
    lo, hi = max(R - 0.03, 0.0), R + 0.03
    on_surface = (lo * lo <= r2) & (r2 <= hi * hi)
    counters["off_surface"] = int((alive & ~on_surface).sum())
    alive &= on_surface
    st, ct = capi.eval_math(2, ph["theta"]).astype(np.float64), capi.eval_math(3, ph["theta"]).astype(np.float64)
    sp, cp = capi.eval_math(2, ph["phi"]).astype(np.float64), capi.eval_math(3, ph["phi"]).astype(np.float64)
    dx, dy, dz = st * cp, st * sp, ct
    c = np.where(-dz < 1.0, -dz, 1.0)                   # (c < 1 ? c : 1, then c > -1 ? c : -1: a NaN gives 1, which np.minimum would pass on)
    c = np.where(c > -1.0, c, -1.0)
    k = np.asarray(class_of(ph["stringID"], ph["omID"]), dtype=np.int64)
    counters["unknown_dom"] = int((alive & (k < 0)).sum())
    alive &= k >= 0
    A = np.zeros(len(ph))
    wlen = ph["wavelength"].astype(np.float64)
    for index, (start, step, values) in enumerate(tables):
        values = np.asarray(values, dtype=np.float64)
        q = (wlen - start) / step
        fbin = np.trunc(q)
        frac = q - fbin
        low = (fbin < 0) | ((fbin == 0) & (frac < 0))
        high = ~low & ~(fbin < len(values) - 1)
        fbin = np.where(low, 0.0, np.where(high, len(values) - 2.0, fbin))
        frac = np.where(low, 0.0, np.where(high, 1.0, frac))
        b = fbin.astype(np.int64)
        a = values[b] + (values[b + 1] - values[b]) * frac
        A = np.where(k == index, a, A)
    P = W * A
    total = np.full(len(ph), coefficients[0])
    multiplier = np.ones(len(ph))
    for coefficient in coefficients[1:]:
        multiplier = multiplier * c
        total = total + coefficient * multiplier
    P = P * total
    above = P > 1.0
    counters["probability_above_one"] = int((alive & above).sum())
    alive &= ~above
    h = np.full(len(ph), seed, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(10):
            word = w[:, 2 * j].astype(np.uint64) | (w[:, 2 * j + 1].astype(np.uint64) << np.uint64(32))
            h = _splitmix64(h ^ word)
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    accepted = alive & ~(P <= u)
    dot = (-x) * dx + (-y) * dy + (-z) * dz
    time = ph["t"].astype(np.float64) + dot * (1.0 - pancake / oversize) / ph["groupVelocity"].astype(np.float64)
    time = np.where(np.isnan(time), np.uint64(0x7ff8000000000000).view(np.float64), time)       # a NaN time has one bit pattern
    out = np.zeros(int(accepted.sum()), dtype=CV.MCPE_DTYPE)
    out["id"], out["stringID"], out["omID"], out["time"] = ph["id"][accepted], ph["stringID"][accepted], ph["omID"][accepted], time[accepted]
    return out, counters, P[alive], accepted[alive]


def sort_mcpes(m):
    """canonical order for comparison as multisets"""
    m = np.ascontiguousarray(m, dtype=CV.MCPE_DTYPE)
    return m[np.lexsort((m["time"].view(np.uint64), m["omID"], m["stringID"], m["id"]))]
