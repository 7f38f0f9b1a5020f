"""Shared by tests/test_hit_records.py and tests/test_hit_records_gpu.py: photon records no propagator delivers, for the two hit
makers (MCPE generator, multi-PMT hit generator).  Both accept "any buffer of records with IDs" (include/clsimhip.h), so the host
twin, the numpy restatement and the kernel have to agree on every bit pattern a record can hold, not only on physical ones.

Set A: records of the `mie` and `lea` fixtures with ONE field class edited per disjoint slice (the rest of the record stays valid,
       so that it reaches the deep branches); `id` is the running index, so an output record names its input.
Set B: random bits; half of them with a known DOM, a position on the sphere and a weight in (0, 2].
Set C: PMT maker only: one or two discs built around a record that flies along +z exactly (theta = phi = 0 give the direction
       (0, 0, 1) without rounding), so that the denominator n . d is the disc axis' z component, bit for bit.
All sets are deterministic: a seed and nothing else."""
import functools

import numpy as np

from clsim_amd import converter as CV
from clsim_amd.synthetic import PHOTON_DTYPE
from oracle import capi
from tests import mcpe_common as M
from tests import pmt_common as PC

OVERSIZE = M.OVERSIZE
NEGATIVE_STRINGS = (-4, -3, -2, -1)         # the generators hold DOMs on these too: word 11's low half is a signed 16-bit ID
TWO_O_PI = np.float32(0.636619772367581343)             # detmath.hip.h: TWO_O_PI
SINCOS_2PI_MAX = np.float32(6.2831855)                  # detmath.hip.h: SINCOS_2PI_MAX
CANONICAL_NAN = np.uint64(0x7ff8000000000000)


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)[()]


def step_ulps(x, n):
    """the float n steps away from the float32 x, away from zero for n > 0 (x != 0)"""
    return (np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.int64) + n).astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def first_angle_beyond_int32():
    """the smallest positive float32 x whose quadrant count rint(x * TWO_O_PI) -- formed in binary32, as the Cephes branch forms it --
    is 2^31 or more (about 3.37e9).  The product grows with x, and every float from 2^23 on is an integer."""
    lo, hi = np.float32(3e9).view(np.uint32), np.float32(4e9).view(np.uint32)
    count = lambda bits: np.rint(np.uint32(bits).view(np.float32) * TWO_O_PI)
    assert count(lo) < 2.0 ** 31 <= count(hi)
    while hi - lo > 1:
        mid = np.uint32((int(lo) + int(hi)) // 2)
        lo, hi = (mid, hi) if count(mid) < 2.0 ** 31 else (lo, mid)
    return np.uint32(hi).view(np.float32)


def beyond_int32(angle):
    """the angle's quadrant count is not an int32 (NaN, infinite or huge), among the angles that take the Cephes branch"""
    a = np.asarray(angle, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.rint(a * TWO_O_PI)
        table = (a >= 0) & (a <= SINCOS_2PI_MAX)
        return ~table & ~((k >= -2.0 ** 31) & (k < 2.0 ** 31))


DENORMAL = f32(0x00012345)                  # 1.0e-40
QUIET_NAN, SIGNALLING_NAN = f32(0x7fc00000), f32(0x7f800001)


def angle_values():
    first = first_angle_beyond_int32()
    return [("+0", np.float32(0.0)), ("-0", np.float32(-0.0)), ("denormal", DENORMAL), ("negated", None),
            ("2pi_max-", step_ulps(SINCOS_2PI_MAX, -1)), ("2pi_max", SINCOS_2PI_MAX), ("2pi_max+", step_ulps(SINCOS_2PI_MAX, 1)),
            ("1e5", np.float32(1e5)), ("int32-", step_ulps(first, -1)), ("int32+", first), ("1e10", np.float32(1e10)),
            ("-1e10", np.float32(-1e10)), ("1e30", np.float32(1e30)), ("+inf", np.float32(np.inf)), ("-inf", np.float32(-np.inf)),
            ("qnan", QUIET_NAN), ("snan", SIGNALLING_NAN)]


TIME_VALUES = [("+inf", np.float32(np.inf)), ("-inf", np.float32(-np.inf)), ("-0", np.float32(-0.0)), ("denormal", DENORMAL),
               ("qnan", QUIET_NAN), ("-qnan", f32(0xffc00000)), ("qnan_payload", f32(0x7fc12345)), ("snan", SIGNALLING_NAN),
               ("-snan_payload", f32(0xff80beef))]
VELOCITY_VALUES = [("+0", np.float32(0.0)), ("-0", np.float32(-0.0)), ("denormal", DENORMAL), ("negative", np.float32(-0.22)),
                   ("inf", np.float32(np.inf)), ("nan", QUIET_NAN)]
WEIGHT_VALUES = [("-0", np.float32(-0.0)), ("denormal", DENORMAL), ("inf", np.float32(np.inf)), ("nan", QUIET_NAN),
                 ("above_0", f32(0x00000001)), ("below_0", f32(0x80000001))]


def wavelength_values():
    start, step, values = M.acceptance_table()
    first, last = np.float32(start), np.float32(start + step * (len(values) - 1))
    return [("below", np.float32(1e-7)), ("first-", step_ulps(first, -1)), ("first", first), ("first+", step_ulps(first, 1)),
            ("last-", step_ulps(last, -1)), ("last", last), ("last+", step_ulps(last, 1)), ("beyond", np.float32(9e-7)),
            ("negative", np.float32(-4e-7)), ("denormal", DENORMAL), ("+inf", np.float32(np.inf)), ("-inf", np.float32(-np.inf)),
            ("nan", QUIET_NAN)]


def surface_window(pancake):
    """(lo2, hi2) as the generators form them"""
    R = M.DOM_RADIUS * OVERSIZE / pancake
    lo, hi = max(R - 0.03, 0.0), R + 0.03
    return lo * lo, hi * hi


def r2_of(ph):
    x, y, z = (ph[k].astype(np.float64) for k in "xyz")
    return x * x + y * y + z * z


def on_window_edge(ph, target, ulps):
    """the positions rescaled in binary64 so that r2 lands on `target`, then the largest coordinate moved by `ulps` floats"""
    p = np.stack([ph[k].astype(np.float64) for k in "xyz"], axis=1)
    p = (p * np.sqrt(target / (p * p).sum(axis=1))[:, None]).astype(np.float32)
    rows = np.arange(len(p))
    big = np.abs(p).argmax(axis=1)
    p[rows, big] = step_ulps(p[rows, big], ulps)
    return p


K_ANGLE, K_TIME, K_VELOCITY, K_WEIGHT, K_WAVELENGTH, K_POSITION, K_DOM = 128, 128, 64, 64, 48, 32, 64


@functools.lru_cache(maxsize=None)
def _set_a(pancake):
    base = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea")])
    if pancake != OVERSIZE:                 # the fixtures were recorded with pancake = oversize: move them onto the larger sphere
        for k in "xyz":
            base[k] = base[k] * np.float32(OVERSIZE / pancake)
    lo2, hi2 = surface_window(pancake)
    parts, slices = [], {}
    cursor = [0]

    def take(name, n):
        rows = (cursor[0] + np.arange(n)) % len(base)
        cursor[0] += n
        part = base[rows].copy()
        first = sum(len(p) for p in parts)
        slices[name] = slice(first, first + n)
        parts.append(part)
        return part

    for field in ("theta", "phi"):
        for name, value in angle_values():
            part = take("%s:%s" % (field, name), K_ANGLE)
            part[field] = -part[field] if value is None else value
    for name, value in TIME_VALUES:
        take("t:" + name, K_TIME)["t"] = value
    for name, value in VELOCITY_VALUES:
        take("groupVelocity:" + name, K_VELOCITY)["groupVelocity"] = value
    # two NaN operands meet in the time's sum: which of them an addition passes on differs between x86-64 and gfx950
    part = take("t+groupVelocity:two_nans", K_VELOCITY)
    part["t"], part["groupVelocity"] = f32(0x7fc00001), f32(0xffc00002)
    for name, value in WEIGHT_VALUES:
        take("weight:" + name, K_WEIGHT)["weight"] = value
    for name, value in wavelength_values():
        take("wavelength:" + name, K_WAVELENGTH)["wavelength"] = value
    for edge, target in (("lo2", lo2), ("hi2", hi2)):
        for ulps in (-2, -1, 0, 1, 2):
            part = take("xyz:%s%+d" % (edge, ulps), K_POSITION)
            p = on_window_edge(part, target, ulps)
            part["x"], part["y"], part["z"] = p[:, 0], p[:, 1], p[:, 2]
    for name, value in (("zero", np.float32(0.0)), ("denormal", DENORMAL)):
        part = take("xyz:" + name, K_POSITION)
        part["x"], part["y"], part["z"] = value, value, value
    for name, value in (("inf", np.float32(np.inf)), ("nan", QUIET_NAN)):
        part = take("xyz:" + name, K_POSITION)
        which = np.arange(K_POSITION) % 3
        for i, k in enumerate("xyz"):
            part[k] = np.where(which == i, value, part[k])
    for name, (string, om) in (("unknown_string", (90, 5)), ("unknown_om", (3, 70)), ("unknown_negative", (-100, 5)),
                               ("unknown_extreme", (-32768, 65535)), ("known_negative", (-2, 7))):
        part = take("dom:" + name, K_DOM)
        part["stringID"], part["omID"] = string, om
    records = np.concatenate(parts)
    records["id"] = np.arange(len(records), dtype=np.uint32)
    records.setflags(write=False)
    return records, slices


def set_a(pancake=OVERSIZE):
    """(records, {slice name: slice}) -- left unchanged by every caller (the array is read-only)"""
    return _set_a(float(pancake))


@functools.lru_cache(maxsize=None)
def _set_b(pancake, n, seed):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2 ** 32, size=(n, 20), dtype=np.uint32)
    records = words.view(PHOTON_DTYPE).reshape(n).copy()
    half = records[n // 2:]
    m = len(half)
    s, d = dom_pairs()
    pick = rng.integers(0, len(s), size=m)
    half["stringID"], half["omID"] = s[pick], d[pick]
    v = rng.standard_normal((m, 3))
    v *= (M.DOM_RADIUS * OVERSIZE / pancake) / np.sqrt((v * v).sum(axis=1))[:, None]
    half["x"], half["y"], half["z"] = v[:, 0], v[:, 1], v[:, 2]
    half["weight"] = (2.0 * (1.0 - rng.random(m))).astype(np.float32)           # (0, 2]
    records["id"] = 0x40000000 + np.arange(n, dtype=np.uint32)
    records.setflags(write=False)
    return records


def set_b(pancake=OVERSIZE, n=65536, seed=20261018):
    return _set_b(float(pancake), n, seed)


# ---- the generators the sets are converted with ----
def dom_pairs():
    """the 86 x 60 detector and four strings with negative IDs"""
    s, d = M.all_pairs()
    extra = np.repeat(np.asarray(NEGATIVE_STRINGS, dtype=np.int32), 60)
    return np.concatenate([s, extra]), np.concatenate([d, np.tile(np.arange(60, dtype=np.uint32), len(NEGATIVE_STRINGS))])


def lookup(strings, oms, values):
    """values[i] for the (string ID, OM ID) pairs of dom_pairs(), -1 for any other pair"""
    key = lambda a, b: (np.asarray(a).astype(np.int64) & 0xFFFF) | (np.asarray(b).astype(np.int64) << 16)
    s, d = dom_pairs()
    keys = key(s, d)
    order = np.argsort(keys)
    want = key(strings, oms)
    at = np.minimum(np.searchsorted(keys[order], want), len(keys) - 1)
    return np.where(keys[order][at] == want, np.asarray(values)[order][at], -1)


def mcpe_tables():
    """class 0: the DOM acceptance; class 1: twice that and 0.3 more, so that records whose wavelength lies outside the table (most
    random bit patterns) keep a probability worth drawing against, and fixture records (weight = 1 / acceptance) exceed 1"""
    start, step, values = M.acceptance_table()
    return [(start, step, values), (start, step, values * 2.0 + 0.3)]


def mcpe_class_of(strings, oms):
    s, d = dom_pairs()
    return lookup(strings, oms, s % 2)


def mcpe_generator(pancake=OVERSIZE):
    s, d = dom_pairs()
    return M.make_generator(mcpe_tables(), s, d, (s % 2).astype(np.int32), pancake=pancake)


def restated_mcpes(photons, pancake=OVERSIZE):
    with np.errstate(all="ignore"):
        return M.numpy_mcpes(photons, mcpe_tables(), mcpe_class_of, M.angular_coefficients(), pancake)


def pmt_configuration(rotation):
    """pmt_common's two-type layout (31 and 4 PMTs, by string parity) on dom_pairs(); the second type's quantum efficiency gets
    0.3 more, for the reason given in mcpe_tables()"""
    R = PC.sphere_radius_of("mie")
    functions = PC.standard_functions()
    start, step, values = M.acceptance_table()
    functions[3] = PC.table(start, step, values * 0.6 + 0.3)
    types, pmts = PC.layout(R, two_types=True)
    s, d = dom_pairs()
    modules = np.zeros(len(s), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"], modules["type"] = s, d, s % 2
    modules["rotation"] = np.asarray(PC.TILTED if rotation == "tilted" else PC.IDENTITY, dtype=np.float64).reshape(9)
    return functions, types, pmts, modules


def restated_hits(photons, configuration, seed=PC.SEED):
    with np.errstate(all="ignore"):
        return PC.numpy_pmt_hits(photons, *configuration, seed=seed)


# ---- set C ----
@functools.lru_cache(maxsize=None)
def set_c():
    """[(name, records, configuration)].  Every record sits at p = (0.05, 0, -sqrt(R^2 - 0.05^2)) and flies along d = (0, 0, 1): the
    denominator of disc i is its axis' z component, the numerator (a - p) . n.  The module's rotation is the identity.
      denom_zero        axis (1, 0, 0), centre off the ray's plane: mu = +inf
      denom_below       axis (1, 0, 1e-8 less one float): below the threshold, met from behind (c < 0): found, then dropped
      denom_at          axis (1, 0, 1e-8): at the threshold, the disc is skipped
      denom_front       axis (1, 0, -1e-8): met from the front at c = 1e-8, drawn like any other
      nan_path_first    disc 0 gives mu = 0 / 0 (axis (1, 0, 0), centre in the ray's plane), disc 1 a plain intersection 3 cm ahead: the NaN
                        path length makes the later disc replace the earlier one (the `path != path` rule)
      nan_path_second   the same discs the other way round: mu < path is false for a NaN, the plain disc stays
      equal_mu          two discs in one plane, both met: equal mu, the first stays"""
    R = PC.sphere_radius_of("mie")
    base = M.fixture_photons("mie")[:1]
    x0 = np.float32(0.05)
    z0 = np.float32(-np.sqrt(R * R - float(x0) ** 2))
    px, pz = float(x0), float(z0)

    def records(n, first_id):
        ph = np.repeat(base, n)
        ph["x"], ph["y"], ph["z"], ph["theta"], ph["phi"] = x0, 0.0, z0, 0.0, 0.0
        ph["id"] = first_id + np.arange(n, dtype=np.uint32)
        ph.setflags(write=False)
        return ph

    def discs(*axes_and_centres):
        types = np.zeros(1, dtype=CV.PMT_TYPE_DTYPE)
        types[0] = (R, 0, len(axes_and_centres), 0, 0)
        pmts = np.zeros(len(axes_and_centres), dtype=CV.PMT_DTYPE)
        for i, (n, a) in enumerate(axes_and_centres):
            pmts["axis"][i], pmts["position"][i] = n, a
        pmts["radius"], pmts["collectionEfficiency"] = 0.30 * R, 0.9
        pmts["quantumEfficiency"], pmts["angularAcceptance"] = 1, 2
        return PC.standard_functions(), types, pmts, PC.modules_for(PC.IDENTITY)

    zero = np.array([float(capi.eval_math(k, np.zeros(1, dtype=np.float32))[0]) for k in (2, 3)])
    assert zero[0] == 0.0 and zero[1] == 1.0             # sin 0, cos 0: the direction is (0, 0, 1) exactly
    in_plane, ahead = (px, 0.0, pz + 0.02), (px, 0.0, pz + 0.03)
    below = float(np.nextafter(1e-8, 0.0))
    cases = [("denom_zero", 16, discs(((1.0, 0.0, 0.0), (px + 0.001, 0.0, pz + 0.02)))),
             ("denom_below", 16, discs(((1.0, 0.0, below), in_plane))),
             ("denom_at", 16, discs(((1.0, 0.0, 1e-8), in_plane))),
             ("denom_front", 64, discs(((1.0, 0.0, -1e-8), in_plane))),
             ("nan_path_first", 64, discs(((1.0, 0.0, 0.0), in_plane), ((0.0, 0.0, -1.0), ahead))),
             ("nan_path_second", 64, discs(((0.0, 0.0, -1.0), ahead), ((1.0, 0.0, 0.0), in_plane))),
             ("equal_mu", 64, discs(((0.0, 0.0, -1.0), ahead), ((0.0, 0.0, -1.0), (px + 0.01, 0.0, pz + 0.03))))]
    return [(name, records(n, 0x20000000 + 0x1000 * i), configuration) for i, (name, n, configuration) in enumerate(cases)]


# ---- the generators at their limits ----
def full_pmt_case():
    """(records, configuration) with 8 types x 64 PMTs, 64 functions of 48 table values each (3 072 together): type = string index
    mod 8; type t has glass / gel function 8 t, quantum efficiency 8 t + 7 (so function 63 serves type 7, and its table lies last in
    the value array) and the shared angular acceptance, function 1; the other functions are never read.  Records: `mie` and `lea`,
    then 256 of them with a wavelength beyond every table, which read each table's last value."""
    R = PC.sphere_radius_of("mie")
    start, step, values = M.acceptance_table()
    q48 = np.interp(start + step * 42 * np.arange(48) / 47.0, start + step * np.arange(43), values)
    c = np.linspace(0.0, 1.0, 48)
    functions = []
    for f in range(64):
        if f == 1:
            functions.append(PC.table(0.0, 1.0 / 47.0, c * (0.2 + 0.6 * c)))
        elif f % 8 == 0:
            functions.append(PC.table(260e-9, 420e-9 / 47.0, np.linspace(0.80, 0.95, 48) - 0.01 * (f // 8)))
        elif f % 8 == 7:
            functions.append(PC.table(start, step * 42 / 47.0, q48 * (1.0 - 0.01 * (f // 8)) + 0.05))
        else:
            functions.append(PC.table(0.0, 1.0, np.full(48, float(f))))
    assert len(functions) == 64 and sum(len(f[3]) for f in functions) == 3072
    types = np.zeros(8, dtype=CV.PMT_TYPE_DTYPE)
    pmts = np.zeros(8 * 64, dtype=CV.PMT_DTYPE)
    axes = PC.fibonacci_axes(64)
    for t in range(8):
        types[t] = (R, 64 * t, 64, 8 * t, 0)
        block = pmts[64 * t:64 * t + 64]
        block["axis"], block["position"], block["radius"] = axes, 0.85 * R * axes, 0.30 * R
        block["collectionEfficiency"], block["quantumEfficiency"], block["angularAcceptance"] = 0.9 - 0.01 * t, 8 * t + 7, 1
    s, d = M.all_pairs()
    modules = np.zeros(len(s), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"], modules["type"] = s, d, s % 8
    modules["rotation"] = PC.TILTED.reshape(9)
    base = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea")])
    beyond = base[:256].copy()
    beyond["wavelength"] = np.float32(9e-7)
    records = np.concatenate([base, beyond])
    records["id"] = np.arange(len(records), dtype=np.uint32)
    return records, (functions, types, pmts, modules)


def full_mcpe_case():
    """(records, tables, class_of, generator) with 8 classes of 512 values each, 4 096 together; class = string index mod 8; class
    7's table lies last.  Records as in full_pmt_case()."""
    start, step, values = M.acceptance_table()
    fine = np.interp(start + step * 42 * np.arange(512) / 511.0, start + step * np.arange(43), values)
    tables = [(start, step * 42 / 511.0, fine * (1.0 - 0.05 * k) + 1e-4 * k) for k in range(8)]
    s, d = M.all_pairs()
    gen = M.make_generator(tables, s, d, (s % 8).astype(np.int32))
    class_of = lambda strings, oms: np.where((np.asarray(strings) >= 0) & (np.asarray(strings) < 86) & (np.asarray(oms) < 60), np.asarray(strings) % 8, -1)
    base = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea")])
    beyond = base[:256].copy()
    beyond["wavelength"] = np.float32(9e-7)
    records = np.concatenate([base, beyond])
    records["id"] = np.arange(len(records), dtype=np.uint32)
    return records, tables, class_of, gen


# ---- the stride loop ----
STRIDE_N = 2 * 262144 + 3 * 64 + 17


@functools.lru_cache(maxsize=None)
def stride_records():
    """524 497 records: the `mie` fixture tiled, word 10 (`id`) the running index"""
    base = M.fixture_photons("mie")
    records = np.tile(base, STRIDE_N // len(base) + 1)[:STRIDE_N].copy()
    records["id"] = np.arange(STRIDE_N, dtype=np.uint32)
    records.setflags(write=False)
    return records
