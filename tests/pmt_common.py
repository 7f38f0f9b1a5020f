"""Shared by tests/test_pmt_hits.py and tests/test_pmt_hits_gpu.py: one synthetic multi-PMT layout for the committed photon
records of tests/mcpe_common.py, and an independent numpy restatement of the hit maker's definition (include/clsimhip.h,
"Multi-PMT hit generator").

The layout: 31 PMTs whose axes lie on a Fibonacci sphere, disc centres at 0.85 R along the axis, disc radius 0.30 R, on a sphere
of R = 0.1651 m (0.8255 m for the records of `lea_no_pancake`, which were taken without the pancake factor).  Neighbouring discs
overlap as seen along a ray, so that every fixture holds records that meet two of them."""
import numpy as np

from clsim_amd import converter as CV
from clsim_amd.synthetic import PHOTON_DTYPE
from oracle import capi
from tests import mcpe_common as M

FIXTURES = M.FIXTURES
SEED = M.SEED
MASK = M.MASK


def sphere_radius_of(name):
    return M.DOM_RADIUS * M.OVERSIZE / M.pancake_of(name)


def fibonacci_axes(n):
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    axes = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    return axes / np.sqrt((axes * axes).sum(axis=1))[:, None]


def rotation_about(axis, angle):
    """Rodrigues: row-major 3 x 3, module frame -> detector frame"""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.sqrt((k * k).sum())
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


IDENTITY = np.eye(3)
TILTED = rotation_about((1.0, 2.0, 3.0), 0.7)


def table(start, step, values):
    return ("table", float(start), float(step), np.asarray(values, dtype=np.float64))


def constant(value):
    return ("constant", float(value))


def standard_functions(q_scale=1.0):
    """[0] G: glass / gel survival over the wavelength; [1] Q: the DOM's wavelength acceptance, which the records' weights are the
    inverse of; [2] A: angular acceptance factor over c, c (0.2 + 0.6 c) on eleven points; [3] Q of the second type: 0.6 Q"""
    start, step, values = M.acceptance_table()
    c = np.linspace(0.0, 1.0, 11)
    return [table(260e-9, 20e-9, np.linspace(0.80, 0.95, 23)), table(start, step, values * q_scale), table(0.0, 0.1, c * (0.2 + 0.6 * c)),
            table(start, step, values * 0.6 * q_scale)]


def layout(R, two_types=False):
    """(types, pmts): type 0 has 31 PMTs; with two_types type 1 has 4 (other quantum efficiency, other collection efficiency)"""
    counts = (31, 4) if two_types else (31,)
    types = np.zeros(len(counts), dtype=CV.PMT_TYPE_DTYPE)
    pmts = np.zeros(sum(counts), dtype=CV.PMT_DTYPE)
    first = 0
    for t, n in enumerate(counts):
        types[t] = (R, first, n, 0, 0)
        axes = fibonacci_axes(n)
        block = pmts[first:first + n]
        block["axis"] = axes
        block["position"] = 0.85 * R * axes
        block["radius"] = 0.30 * R
        block["collectionEfficiency"] = 0.9 if t == 0 else 0.8
        block["quantumEfficiency"] = 1 if t == 0 else 3
        block["angularAcceptance"] = 2
        first += n
    return types, pmts


def modules_for(rotation, two_types=False, strings=None):
    """every (string index, DOM index) of the 86 x 60 detector, type by string parity with two types"""
    s, d = M.all_pairs()
    if strings is not None:
        keep = np.isin(s, strings)
        s, d = s[keep], d[keep]
    modules = np.zeros(len(s), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"] = s, d
    modules["type"] = (s % 2) if two_types else 0
    modules["rotation"] = np.asarray(rotation, dtype=np.float64).reshape(9)
    return modules


CONFIGURATIONS = ("identity", "tilted", "two_types")


def configuration(name, R, q_scale=1.0, strings=None):
    """(functions, types, pmts, modules) of one of the three configurations the tests run"""
    two = name == "two_types"
    types, pmts = layout(R, two)
    return standard_functions(q_scale), types, pmts, modules_for(TILTED if name == "tilted" else IDENTITY, two, strings)


def function_object(f):
    return CV.I3CLSimFunctionFromTable(f[1], f[2], f[3]) if f[0] == "table" else CV.I3CLSimFunctionConstant(f[1])


def make_generator(functions, types, pmts, modules, seed=SEED):
    return CV.PMTHitGenerator([function_object(f) for f in functions], types, pmts, modules, seed=seed)


def evaluate(f, x):
    """FromTable with equal spacing (clamped to the first / last bin) or Constant, in binary64"""
    if f[0] == "constant":
        return np.full(len(x), f[1])
    _, start, step, values = f
    q = (x - start) / step
    fbin = np.trunc(q)
    frac = q - fbin
    low = (fbin < 0) | ((fbin == 0) & (frac < 0))
    high = ~low & ~(fbin < len(values) - 1)
    fbin = np.where(low, 0.0, np.where(high, len(values) - 2.0, fbin))
    frac = np.where(low, 0.0, np.where(high, 1.0, frac))
    b = fbin.astype(np.int64)
    return values[b] + (values[b + 1] - values[b]) * frac


def numpy_pmt_hits(photons, functions, types, pmts, modules, seed=SEED):
    """The definition once more, in numpy binary64 (the two sin / cos pairs come from the oracle's C restatement of the device math
    library).  Returns (hits in input order, counters dict, details): details holds per record `found` (PMT index or -1), `double`
    (the record met two discs or more), `c`, `P` and the masks `drawn` (reached the draw) and `accepted`."""
    ph = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
    n = len(ph)
    w = ph.view(np.uint32).reshape(n, 20)
    types = np.asarray(types, dtype=CV.PMT_TYPE_DTYPE)
    pmts = np.asarray(pmts, dtype=CV.PMT_DTYPE)
    modules = np.asarray(modules, dtype=CV.PMT_MODULE_DTYPE)
    counters = dict.fromkeys(CV.PMT_CONDITIONS, 0)
    # module of every record: by (string ID, OM ID)
    key_of = lambda s, d: (np.asarray(s).astype(np.int64) & 0xFFFF) | (np.asarray(d).astype(np.int64) << 16)
    order = np.argsort(key_of(modules["stringID"], modules["omID"]), kind="stable")
    keys = key_of(modules["stringID"], modules["omID"])[order]
    want = key_of(ph["stringID"], ph["omID"])
    at = np.minimum(np.searchsorted(keys, want), max(len(keys) - 1, 0))
    known = (keys[at] == want) if len(keys) else np.zeros(n, dtype=bool)
    counters["unknown_module"] = int((~known).sum())
    module = np.where(known, order[at] if len(keys) else 0, 0)
    m = modules["rotation"][module] if len(modules) else np.zeros((n, 9))
    kind = np.where(known, modules["type"][module] if len(modules) else 0, -1)
    px, py, pz = (ph[k].astype(np.float64) for k in ("x", "y", "z"))
    st, ct = capi.eval_math(2, ph["theta"]).astype(np.float64), capi.eval_math(3, ph["theta"]).astype(np.float64)
    sp, cp = capi.eval_math(2, ph["phi"]).astype(np.float64), capi.eval_math(3, ph["phi"]).astype(np.float64)
    dx, dy, dz = st * cp, st * sp, ct
    entering = known & ~((px * dx + py * dy + pz * dz) > 0.0)
    pr2 = px * px + py * py + pz * pz
    found = np.full(n, -1, dtype=np.int64)
    crossings = np.zeros(n, dtype=np.int64)
    path = np.zeros(n)
    rx, ry, rz = np.zeros(n), np.zeros(n), np.zeros(n)
    q_of, a_of, ce = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
    g_of = np.zeros(n, dtype=np.int64)
    off_surface = np.zeros(n, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t, T in enumerate(types):
            mine = entering & (kind == t)
            R = float(T["sphereRadius"])
            lo, hi = max(R - 0.03, 0.0), R + 0.03
            off_surface |= mine & ~((lo * lo <= pr2) & (pr2 <= hi * hi))
            g_of[mine] = T["glassGelSurvival"]
            for i in range(int(T["numPMTs"])):
                E = pmts[int(T["firstPMT"]) + i]
                v = E["axis"]
                nx = (m[:, 0] * v[0] + m[:, 1] * v[1]) + m[:, 2] * v[2]
                ny = (m[:, 3] * v[0] + m[:, 4] * v[1]) + m[:, 5] * v[2]
                nz = (m[:, 6] * v[0] + m[:, 7] * v[1]) + m[:, 8] * v[2]
                denom = dx * nx + dy * ny + dz * nz
                ok = mine & ~(denom >= 1e-8)
                v = E["position"]
                ax = (m[:, 0] * v[0] + m[:, 1] * v[1]) + m[:, 2] * v[2]
                ay = (m[:, 3] * v[0] + m[:, 4] * v[1]) + m[:, 5] * v[2]
                az = (m[:, 6] * v[0] + m[:, 7] * v[1]) + m[:, 8] * v[2]
                mu = ((ax - px) * nx + (ay - py) * ny + (az - pz) * nz) / denom
                ok &= ~(mu < 0.0)
                ex, ey, ez = ax - px - mu * dx, ay - py - mu * dy, az - pz - mu * dz
                ok &= ~((ex * ex + ey * ey + ez * ez) > float(E["radius"]) * float(E["radius"]))
                crossings += ok
                take = ok & ((found < 0) | np.isnan(path) | (mu < path))
                found = np.where(take, i, found)
                path = np.where(take, mu, path)
                rx, ry, rz = np.where(take, nx, rx), np.where(take, ny, ry), np.where(take, nz, rz)
                q_of = np.where(take, E["quantumEfficiency"], q_of)
                a_of = np.where(take, E["angularAcceptance"], a_of)
                ce = np.where(take, E["collectionEfficiency"], ce)
        counters["off_surface"] = int(off_surface.sum())
        c = -(rx * dx + ry * dy + rz * dz)
        alive = (found >= 0) & ~(c <= 0.0)
        wlen = ph["wavelength"].astype(np.float64)
        pick = lambda index, x: np.select([index == k for k in range(len(functions))], [evaluate(f, x) for f in functions], 0.0)
        P = ph["weight"].astype(np.float64)
        P = P * pick(g_of, wlen)
        P = P * (pick(q_of, wlen) * ce)
        P = P * (pick(a_of, c) / c)
    above = alive & (P > 1.0)
    counters["probability_above_one"] = int(above.sum())
    drawn = alive & ~above
    h = np.full(n, seed, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(10):
            word = w[:, 2 * j].astype(np.uint64) | (w[:, 2 * j + 1].astype(np.uint64) << np.uint64(32))
            h = M._splitmix64(h ^ word)
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    accepted = drawn & ~(P <= u)
    out = np.zeros(int(accepted.sum()), dtype=CV.PMT_HIT_DTYPE)
    out["id"], out["stringID"], out["omID"] = ph["id"][accepted], ph["stringID"][accepted], ph["omID"][accepted]
    out["pmt"], out["time"] = found[accepted], ph["t"][accepted].astype(np.float64)
    details = dict(found=found, double=crossings >= 2, c=c, P=P, drawn=drawn, accepted=accepted, entering=entering)
    return out, counters, details


def geometry_modules(cfg, rotation=IDENTITY, skip=0):
    """a module of type 0 for every DOM of a test configuration's geometry (tests/common.py: config), but the first `skip`"""
    g = cfg["geom"]
    s, d = np.asarray(g["string_ids"])[skip:], np.asarray(g["dom_ids"])[skip:]
    modules = np.zeros(len(s), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"] = s, d
    modules["rotation"] = np.asarray(rotation, dtype=np.float64).reshape(9)
    return modules


def geometry_generator(cfg, R=None, rotation=IDENTITY, skip=0, q_scale=1.0):
    types, pmts = layout(M.DOM_RADIUS if R is None else R)
    return make_generator(standard_functions(q_scale), types, pmts, geometry_modules(cfg, rotation, skip))


def check_compile_refusals():
    """what Compile() refuses with a PMT hit generator attached (host side only: nothing here needs a GPU)"""
    import pytest
    from clsim_amd import _lib
    from tests import common
    cfg = common.config("c1")
    g = cfg["geom"]

    def refused(conv, text):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=text) as e:
            conv.Compile()
        assert e.value.code == _lib.ERR_CONFIG

    good = geometry_generator(cfg)
    conv = common.product_converter(cfg, 512, initialize=False)             # pancake factor 5: records at 0.1651 m
    conv.SetPMTHitGenerator(good, True)
    conv.Compile()
    # both hit makers
    ids_s, ids_d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    conv.SetMCPEGenerator(M.make_generator([M.acceptance_table()], ids_s, ids_d, np.zeros(len(ids_s), dtype=np.int32)), True)
    refused(conv, "not both")
    conv.SetMCPEGenerator(None)
    conv.Compile()
    # MCPE series
    conv.SetMCPESeries(True)
    refused(conv, "MCPE series")
    conv.SetMCPESeries(False)
    conv.Compile()
    # a geometry DOM without a module
    conv.SetPMTHitGenerator(geometry_generator(cfg, skip=1), True)
    refused(conv, r"No module configured for OMKey\(%d,%d\)" % (ids_s[0], ids_d[0]))
    # a type made for another radius: 3 cm and a little more; just inside is taken
    conv.SetPMTHitGenerator(geometry_generator(cfg, R=M.DOM_RADIUS + 0.0301), True)
    refused(conv, "sphere radius")
    conv.SetPMTHitGenerator(geometry_generator(cfg, R=M.DOM_RADIUS * 5.0), True)
    refused(conv, "sphere radius")
    conv.SetPMTHitGenerator(geometry_generator(cfg, R=M.DOM_RADIUS - 0.0299), True)
    conv.Compile()
    # histories without photons
    conv.SetPMTHitGenerator(good, False)
    conv.SetPhotonHistoryEntries(4)
    refused(conv, "photon histories need keep_photons")
    conv.SetPMTHitGenerator(good, True)
    conv.Compile()
    # and off again: as without
    conv.SetPMTHitGenerator(None)
    conv.Compile()


def sort_hits(hits):
    """canonical order for comparison as multisets: (id, string, OM, PMT, time bits)"""
    hits = np.ascontiguousarray(hits, dtype=CV.PMT_HIT_DTYPE)
    return hits[np.lexsort((hits["time"].view(np.uint64), hits["pmt"], hits["omID"], hits["stringID"], hits["id"]))]
