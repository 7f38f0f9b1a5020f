"""Shared by tests/test_cable_shadow.py and tests/test_cable_shadow_gpu.py: the cable shadow rule (include/clsimhip.h: "Cable shadow")
once more in numpy binary64, the same geometric statement in rational arithmetic, cylinder sets and records aimed at them.
Everything is deterministic: a seed and nothing else."""
import functools
from fractions import Fraction

import numpy as np

from clsim_amd import converter as CV
from clsim_amd.synthetic import PHOTON_DTYPE
from oracle import capi
from tests import hit_records_common as H
from tests import mcpe_common as M

DISTANCE = 1.0
TILE = 2048                                 # cable_shadow.h: kCableShadowTile
MAX_CYLINDERS = CV.CABLE_SHADOW_MAX_CYLINDERS


# ---- the rule, restated ----
def cylinder_records(top, bottom, radius):
    """A, a, L2, r2 as the library precomputes them"""
    top, bottom = np.asarray(top, dtype=np.float64).reshape(-1, 3), np.asarray(bottom, dtype=np.float64).reshape(-1, 3)
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (len(top),))
    a = top - bottom
    L2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
    return bottom, a, L2, radius * radius


def segments(photons, distance):
    """(P0 [n, 3], d [n, 3]) of the records: the two sin / cos pairs come from the oracle's C restatement of the device math library"""
    ph = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
    with np.errstate(all="ignore"):
        st, ct = capi.eval_math(2, ph["theta"]).astype(np.float64), capi.eval_math(3, ph["theta"]).astype(np.float64)
        sp, cp = capi.eval_math(2, ph["phi"]).astype(np.float64), capi.eval_math(3, ph["phi"]).astype(np.float64)
        direction = np.stack([st * cp, st * sp, ct], axis=1)
        d = distance * direction
        P1 = np.stack([ph[k].astype(np.float64) for k in "xyz"], axis=1)
        return P1 - d, d


def dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def segment_hits(P0, d, A, a, L2, r2):
    """the test of every segment [n] against every cylinder [c]: bool [n, c].  Every branch of the definition as a mask; what a lane
    that has left would have computed is computed and thrown away."""
    with np.errstate(all="ignore"):
        P0, d = P0[:, None, :], d[:, None, :]
        m = P0 - A[None, :, :]
        a = a[None, :, :]
        ma, da = dot(m, a), dot(d, a)
        u1 = ma + da
        miss = ((ma < 0) & (u1 < 0)) | ((ma > L2) & (u1 > L2))
        moving = da != 0
        ta, tb = (0.0 - ma) / da, (L2 - ma) / da
        swap = ta > tb
        ta, tb = np.where(swap, tb, ta), np.where(swap, ta, tb)
        lo = np.where(moving & (ta > 0.0), ta, 0.0)
        hi = np.where(moving & (tb < 1.0), tb, 1.0)
        miss |= np.where(moving, lo > hi, ~((ma >= 0) & (ma <= L2)))
        dd, mm, md = dot(d, d), dot(m, m), dot(m, d)
        al, be, ga = dd * L2 - da * da, md * L2 - ma * da, (mm - r2) * L2 - ma * ma
        t = (0.0 - be) / al
        t = np.where(t < lo, lo, t)
        t = np.where(t > hi, hi, t)
        t = np.where(al > 0, t, lo)
        return ~miss & ((al * t + (be + be)) * t + ga <= 0)


def numpy_flags(photons, cylinders, distance=DISTANCE, block=1 << 21):
    """flags (uint8, 1 = shadowed) of the records against the cylinder set (top, bottom, radius), `block` pairs at a time"""
    A, a, L2, r2 = cylinder_records(*cylinders)
    P0, d = segments(photons, distance)
    flags = np.zeros(len(P0), dtype=np.uint8)
    rows = max(block // len(A), 1)
    for first in range(0, len(P0), rows):
        flags[first:first + rows] = segment_hits(P0[first:first + rows], d[first:first + rows], A, a, L2, r2).any(axis=1)
    return flags


def restated(photons, cylinders, distance=DISTANCE):
    """(flags, lit, counts) as CableShadow.MakeHost gives them"""
    ph = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
    flags = numpy_flags(ph, cylinders, distance)
    return flags, ph[flags == 0], {"tested": len(ph), "shadowed": int(flags.sum())}


# ---- the same statement, exactly ----
def exact_case(P0, d, top, bottom, radius):
    """(hit, |q_min| / (r^2 L2) or None): "the segment P0 + t d, 0 <= t <= 1, meets the solid finite cylinder" in rational arithmetic on
    the binary64 values given.  q(t) = |m + t d|^2 L2 - ((m + t d).a)^2 - r^2 L2 is the radial condition times L2; its minimum over
    the part of [0, 1] between the caps decides.  None: the segment never lies between the caps."""
    F = lambda v: [Fraction(float(x)) for x in v]
    P0, d, top, bottom = F(P0), F(d), F(top), F(bottom)
    r2 = Fraction(float(radius)) ** 2
    a = [t - b for t, b in zip(top, bottom)]
    m = [p - b for p, b in zip(P0, bottom)]
    fdot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
    L2, ma, da = fdot(a, a), fdot(m, a), fdot(d, a)
    lo, hi = Fraction(0), Fraction(1)
    if da != 0:
        ta, tb = sorted(((0 - ma) / da, (L2 - ma) / da))
        lo, hi = max(lo, ta), min(hi, tb)
        if lo > hi:
            return False, None
    elif not 0 <= ma <= L2:
        return False, None
    al, be, ga = fdot(d, d) * L2 - da * da, fdot(m, d) * L2 - ma * da, (fdot(m, m) - r2) * L2 - ma * ma
    t = lo
    if al > 0:
        t = min(max(-be / al, lo), hi)
    q = (al * t + 2 * be) * t + ga
    return q <= 0, float(abs(q) / (r2 * L2))


@functools.lru_cache(maxsize=None)
def exact_family(n=20000, seed=1):
    """(P0, d, top, bottom, radius) of n single-cylinder cases: cylinders about 1 m long (0.5 - 1.5 m) with small tilts and radii of
    1 - 5 cm, 0.3 - 0.5 m from the origin; end points within +-0.6 m, segments 0.1 - 10 m long, directions isotropic"""
    rng = np.random.default_rng(seed)
    azimuth = rng.uniform(0.0, 2.0 * np.pi, n)
    centre = np.stack([np.cos(azimuth), np.sin(azimuth), np.zeros(n)], axis=1) * rng.uniform(0.3, 0.5, n)[:, None]
    centre[:, 2] = rng.uniform(-0.2, 0.2, n)
    axis = np.stack([rng.normal(0.0, 0.05, n), rng.normal(0.0, 0.05, n), np.ones(n)], axis=1)
    axis /= np.sqrt((axis * axis).sum(axis=1))[:, None]
    half = 0.5 * rng.uniform(0.5, 1.5, n)[:, None] * axis
    top, bottom = centre + half, centre - half
    radius = rng.uniform(0.01, 0.05, n)
    P1 = rng.uniform(-0.6, 0.6, (n, 3))
    direction = rng.standard_normal((n, 3))
    direction /= np.sqrt((direction * direction).sum(axis=1))[:, None]
    d = direction * rng.uniform(0.1, 10.0, n)[:, None]
    return P1 - d, d, top, bottom, radius


# ---- cylinder sets ----
def cable_at(azimuth, offset=0.2, half_length=0.5, tilt=(0.0, 0.0)):
    """(top, bottom) of a cable beside a module at the origin: `offset` from its centre at `azimuth`, about vertical"""
    c = np.array([offset * np.cos(azimuth), offset * np.sin(azimuth), 0.0])
    h = np.array([tilt[0], tilt[1], half_length])
    return c + h, c - h


@functools.lru_cache(maxsize=None)
def cylinder_set(n, spread=0.5 * np.pi):
    """n cables (top [n, 3], bottom [n, 3], radius [n]) beside a module at the origin -- the records' positions are relative to their
    module -- one per DOM of a detector: azimuths spread over `spread`, small tilts, radii about 2.3 cm"""
    rng = np.random.default_rng(1000 + n)
    azimuth = spread * (np.arange(n) + 0.5) / n
    tops, bottoms = zip(*(cable_at(az, tilt=rng.normal(0.0, 0.01, 2)) for az in azimuth))
    out = np.array(tops), np.array(bottoms), 0.023 + 0.002 * rng.random(n)
    for array in out:
        array.setflags(write=False)
    return out


def make_shadow(cylinders, distance=DISTANCE):
    return CV.CableShadow(*cylinders, distance)


# ---- records ----
def aimed_records(cylinders, n, seed, distance=DISTANCE):
    """n records aimed at and past the cylinders: a point near a cylinder's axis (beyond its caps for some, up to three radii off), a
    direction, and the record's position such that the point lies on the line of its last path: inside the segment, before its start or
    beyond its end.  `id` is the running index."""
    top, bottom, radius = cylinders
    rng = np.random.default_rng(seed)
    which = rng.integers(0, len(top), n)
    u = rng.uniform(-0.2, 1.2, n)[:, None]
    near = bottom[which] + u * (top[which] - bottom[which]) + rng.standard_normal((n, 3)) * (radius[which] * rng.uniform(0.0, 1.5, n))[:, None]
    cos_theta = rng.uniform(-1.0, 1.0, n)
    theta, phi = np.arccos(cos_theta).astype(np.float32), rng.uniform(0.0, 2.0 * np.pi, n).astype(np.float32)
    direction = np.stack([np.sin(theta.astype(np.float64)) * np.cos(phi.astype(np.float64)), np.sin(theta.astype(np.float64)) * np.sin(phi.astype(np.float64)),
                          np.cos(theta.astype(np.float64))], axis=1)
    P1 = near + direction * (distance * rng.uniform(-0.5, 1.5, n))[:, None]
    ph = np.repeat(M.fixture_photons("mie")[:1], n)
    ph["x"], ph["y"], ph["z"], ph["theta"], ph["phi"] = P1[:, 0], P1[:, 1], P1[:, 2], theta, phi
    ph["id"] = np.arange(n, dtype=np.uint32)
    return ph


@functools.lru_cache(maxsize=None)
def adversarial_records():
    """hit_records_common's set A (one field class edited per slice: NaNs, infinities, angles beyond the int32 quadrant range) and
    8 192 records of its set B (random bits; half of them with a position on the sphere); read-only"""
    records = np.concatenate([H.set_a()[0], H.set_b()[:4096], H.set_b()[-4096:]])
    records.setflags(write=False)
    return records


@functools.lru_cache(maxsize=None)
def mixed_records(n_cylinders, n=6000, seed=5):
    """fixture records, records aimed at the set, and adversarial ones, interleaved by a fixed permutation; read-only"""
    cylinders = cylinder_set(n_cylinders)
    parts = [M.fixture_photons("mie"), M.fixture_photons("lea"), aimed_records(cylinders, n, seed), adversarial_records()[::7]]
    records = np.concatenate(parts)
    records = records[np.random.default_rng(seed).permutation(len(records))]
    records.setflags(write=False)
    return records


@functools.lru_cache(maxsize=None)
def reference(n_cylinders, which="mixed"):
    """(records, flags, lit, counts) by the restatement, computed once and shared; read-only"""
    records = mixed_records(n_cylinders) if which == "mixed" else adversarial_records()
    flags, lit, counts = restated(records, cylinder_set(n_cylinders))
    flags.setflags(write=False)
    lit.setflags(write=False)
    return records, flags, lit, counts
