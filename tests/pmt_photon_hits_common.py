"""Shared by tests/test_pmt_photon_hits.py, tests/test_pmt_photon_hits_gpu.py and tests/test_pmt_photon_hits_adapter.py: an independent
numpy restatement of the PMT photon hits definition (include/clsimhip.h, "PMT photon hits") -- the series search as the bisection it is
defined as, the geometry and the probability of tests/pmt_common.numpy_pmt_hits on the frame record's fields, the draw over the
record's 48 bytes, np.lexsort for the order -- and the inputs the tests use, all made from committed material: the golden photon
records and tests/frame_photons_common.py's synthetic ones, run through the frame photons stage's host twin."""
import functools
import struct

import numpy as np

from clsim_amd import converter as CV
from tests import frame_photons_common as F
from tests import mcpe_common as M
from tests import photon_hits_common as PH
from tests import pmt_common as PC
from tests import pmt_series_common as PS

U64 = np.uint64
SEED = PC.SEED
COUNTERS = CV.PMT_PHOTON_HIT_COUNTERS


def as_photons(records):
    """the fields the geometry reads, in the 80-byte layout tests/pmt_common.numpy_pmt_hits takes"""
    r = np.ascontiguousarray(records, dtype=CV.FRAME_PHOTON_DTYPE)
    ph = np.zeros(len(r), dtype=CV.PHOTON_DTYPE)
    for name in ("x", "y", "z", "theta", "phi", "wavelength", "weight", "id", "stringID", "omID"):
        ph[name] = r[name]
    return ph


def numpy_hits(records, series, functions, types, pmts, modules, seed=SEED):
    """(hits, series, counters) of the definition"""
    r = np.ascontiguousarray(records, dtype=CV.FRAME_PHOTON_DTYPE)
    t = np.ascontiguousarray(series, dtype=CV.MCPE_SERIES_DTYPE)
    n = len(r)
    counters = dict.fromkeys(COUNTERS, 0)
    owner = PH.series_of(t["first"], n) if len(t) else np.full(n, -1, dtype=np.int64)
    entry = t[np.maximum(owner, 0)] if len(t) else np.zeros(n, dtype=CV.MCPE_SERIES_DTYPE)
    i = np.arange(n, dtype=np.int64)
    uncovered = (owner < 0) | (i - entry["first"].astype(np.int64) >= entry["count"].astype(np.int64))
    counters["uncovered"] = int(uncovered.sum())
    mismatch = ~uncovered & ((r["stringID"] != entry["stringID"]) | (r["omID"] != entry["omID"]))
    counters["series_mismatch"] = int(mismatch.sum())
    alive = np.flatnonzero(~uncovered & ~mismatch)
    r, owner, entry = r[alive], owner[alive], entry[alive]
    _, geometry, details = PC.numpy_pmt_hits(as_photons(r), functions, types, pmts, modules, seed)
    for name in ("unknown_module", "probability_above_one", "off_surface"):
        counters[name] = geometry[name]
    words = r.view(U64).reshape(len(r), 6)
    h = np.full(len(r), seed, dtype=U64)
    with np.errstate(over="ignore"):
        for j in range(6):
            h = M._splitmix64(h ^ words[:, j])
    u = (h >> U64(11)).astype(np.float64) * 2.0 ** -53
    with np.errstate(invalid="ignore"):
        kept = np.flatnonzero(details["drawn"] & ~(details["P"] <= u))
    pmt = details["found"][kept]
    kept = kept[np.lexsort((r["id"][kept], PS.tkey_of(r["time"][kept]), pmt, owner[kept]))]
    pmt, group = details["found"][kept], owner[kept]
    out = np.zeros(len(kept), dtype=CV.PMT_HIT_DTYPE)
    out["id"], out["stringID"], out["omID"], out["pmt"] = r["id"][kept], entry["stringID"][kept], entry["omID"][kept], pmt
    out["time"].view(U64)[:] = r["time"][kept].view(U64)               # bit for bit
    head = np.ones(len(kept), dtype=bool)
    head[1:] = (group[1:] != group[:-1]) | (pmt[1:] != pmt[:-1])
    first = np.flatnonzero(head)
    out_series = np.zeros(len(first), dtype=CV.PMT_SERIES_DTYPE)
    source = t[group[first]] if len(first) else t[:0]
    out_series["frame"], out_series["stringID"], out_series["omID"] = source["frame"], source["stringID"], source["omID"]
    out_series["pmt"], out_series["first"] = pmt[first], first
    out_series["count"] = np.diff(np.append(first, len(kept)))
    return out, out_series, counters


def same(got, want):
    """hits, series and counters, arrays as they are"""
    assert got[2] == want[2]
    for g, w in zip(got[:2], want[:2]):
        assert g.dtype == w.dtype and len(g) == len(w) and g.tobytes() == w.tobytes()


def check_properties(hits, series, in_series):
    """from the arrays alone: the entries partition the hits; (input series, pmt) ascends strictly over the table, where the input
    series of an entry is found by its (frame, module) in the input table; inside an entry (tkey, identifier) does not descend, and
    neighbours equal in it are byte-identical; reserved words are 0"""
    assert int(series["count"].sum()) == len(hits)
    assert np.array_equal(series["first"], np.cumsum(series["count"].astype(np.int64)) - series["count"])
    assert (series["count"] > 0).all() and (series["reserved"] == 0).all() and (hits["reserved"] == 0).all()
    code = lambda s: s["frame"].astype(np.int64) * 2 ** 32 + PS.module_code(s["stringID"], s["omID"])
    position = {c: k for k, c in enumerate(code(in_series).tolist())}
    assert len(position) == len(in_series)
    s_of = np.array([position[c] for c in code(series).tolist()], dtype=np.int64)
    assert (np.diff(s_of * 64 + series["pmt"].astype(np.int64)) > 0).all() and (series["pmt"] < 64).all()
    owner = np.repeat(np.arange(len(series)), series["count"])
    assert np.array_equal(hits["stringID"], series["stringID"][owner]) and np.array_equal(hits["omID"], series["omID"][owner])
    assert np.array_equal(hits["pmt"], series["pmt"][owner])
    t = PS.tkey_of(hits["time"])
    inner = owner[1:] == owner[:-1]
    assert (t[1:][inner] >= t[:-1][inner]).all()
    tie = inner & (t[1:] == t[:-1])
    assert (hits["id"][1:][tie] >= hits["id"][:-1][tie]).all()
    equal = tie & (hits["id"][1:] == hits["id"][:-1])
    raw = hits.view(np.uint8).reshape(len(hits), -1)
    assert (raw[1:][equal] == raw[:-1][equal]).all()


def shuffled_within_series(records, series, seed):
    out = records.copy()
    rng = np.random.default_rng(seed)
    for first, count in zip(series["first"], series["count"]):
        out[first:first + count] = records[first + rng.permutation(count)]
    return out


# ---- inputs ----
def busiest_module(photons):
    codes = PS.module_code(photons["stringID"], photons["omID"])
    values, counts = np.unique(codes, return_counts=True)
    busiest = int(values[counts.argmax()])
    return busiest // 65536 - 32768, busiest % 65536


def fixture_bunch(name):
    """(particle table, mask) for the golden photon records of `name`: three frames with interleaved identifiers and shifts (one frame
    where the fixture has one identifier), and the busiest module masked in each of them"""
    photons = M.fixture_photons(name)
    sid, oid = busiest_module(photons)
    return F.particle_table(photons["id"]), F.mask_of([(f, sid, oid) for f in (7, 2, 900)] + [(5, sid, oid), (7, 99, 99)])


@functools.lru_cache(maxsize=None)
def fixture_records(name, nan_weights=False):
    """the golden photon records of `name` as frame photons, with fixture_bunch's table and mask (nan_weights: every weight a NaN,
    under which the hit maker accepts exactly the photons that meet a PMT from the front, whatever the draw)"""
    photons = M.fixture_photons(name).copy()
    if nan_weights:
        photons["weight"] = np.nan
    strings, oms = M.all_pairs()
    p, masked = fixture_bunch(name)
    records, series, counters = CV.FramePhotonDoms(strings, oms).MakeFramePhotonsHost(photons, p, masked)
    assert counters["unknown_particle"] == 0 == counters["unknown_dom"] == counters["tie_overflow"] and len(records) > 0
    return records, series


SPECIAL_TIME_BITS = (0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001,
                     0x7FF0000000000001, 0xFFF4000000000002)        # +-0, +-inf, quiet NaNs of both signs, signalling NaNs of both signs


def on_the_sphere(records, R, seed, tilt=0.35):
    """the records moved onto the sphere of radius R around their module, flying inwards: position R e, direction -e turned by up to
    `tilt` radians, so that most of them meet a PMT of a Fibonacci layout from the front"""
    r = records.copy()
    rng = np.random.default_rng(seed)
    n = len(r)
    e = rng.standard_normal((n, 3))
    e /= np.linalg.norm(e, axis=1)[:, None]
    d = -e + tilt * rng.uniform(-1.0, 1.0, (n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r["x"], r["y"], r["z"] = (R * e).T
    r["theta"] = np.arccos(np.clip(d[:, 2], -1.0, 1.0))
    r["phi"] = np.arctan2(d[:, 1], d[:, 0]) % (2.0 * np.pi)
    return r


@functools.lru_cache(maxsize=None)
def synthetic_records(n, seed, special_times=True, weight=None):
    """frame photons at the synthetic modules of tests/pmt_series_common.py (its DOM list is frame_photons_common's), on the sphere
    and flying inwards; special_times: the eight patterns of SPECIAL_TIME_BITS, a few of each, put in after the frame photons stage
    (which would quiet a signalling NaN)"""
    photons = F.synthetic_photons(n, seed, special=False)
    if weight is not None:
        photons["weight"] = weight
    records, series, counters = F.synthetic_doms().MakeFramePhotonsHost(photons, F.particle_table(photons["id"]))
    assert len(records) == n and not any(counters.values())
    records = on_the_sphere(records, PS.RADIUS, seed + 500)
    if special_times and n >= 64:
        at = np.random.default_rng(seed + 9).choice(n, 32, replace=False)
        records["time"].view(U64)[at] = np.tile(np.array(SPECIAL_TIME_BITS, dtype=U64), 4)
    return records, series


def aim(records, seed, pmt=None, n_pmts=(31, 64)):
    """in place: every record on the sphere within 0.09 R of the axis of one PMT of its module's type (pmt: which, default any),
    flying against the axis; returns the PMT numbers"""
    n = len(records)
    rng = np.random.default_rng(seed)
    kind = records["stringID"].astype(np.int64) % len(n_pmts)
    which = (rng.integers(0, 1 << 30, n) % np.asarray(n_pmts)[kind]) if pmt is None else np.full(n, pmt)
    axes = np.zeros((n, 3))
    for t, count in enumerate(n_pmts):
        axes[kind == t] = PC.fibonacci_axes(count)[which[kind == t]]
    e = axes + 0.05 * rng.uniform(-1.0, 1.0, (n, 3))
    e /= np.linalg.norm(e, axis=1)[:, None]
    records["x"], records["y"], records["z"] = (PS.RADIUS * e).T
    records["theta"] = np.arccos(np.clip(-axes[:, 2], -1.0, 1.0))
    records["phi"] = np.arctan2(-axes[:, 1], -axes[:, 0]) % (2.0 * np.pi)
    return which


def aimed_records(n, seed, counts=None, pmt=None, special_times=False, n_pmts=(31, 64)):
    """n frame photons of weight 1 at the synthetic modules (counts: counts[k] of them at the k-th module of frame_photons_common's list,
    one frame), each aimed at one PMT of its module's type in a keep_all_layout with the identity rotation (pmt: which, default any):
    on the sphere within 0.09 R of the PMT's axis, flying against the axis.  Every one of them makes a hit on that PMT."""
    photons = F.synthetic_photons(n, seed, special=False, quantised=False)
    photons["weight"] = 1.0
    if counts is not None:
        module = np.repeat(np.arange(len(counts)), counts)
        photons["stringID"], photons["omID"] = F.DOM_STRINGS[module], F.DOM_OMS[module]
    records, series, counters = F.synthetic_doms().MakeFramePhotonsHost(photons, None if counts is not None else F.particle_table(photons["id"]))
    assert len(records) == n and not any(counters.values())
    which = aim(records, seed + 77, pmt, n_pmts)
    if special_times and n >= 64:
        at = np.random.default_rng(seed + 9).choice(n, 32, replace=False)
        records["time"].view(U64)[at] = np.tile(np.array(SPECIAL_TIME_BITS, dtype=U64), 4)
    return records, series, which


def synthetic_layout(ce=0.9, radius_fraction=0.2):
    """tests/pmt_series_common.synthetic_layout (31 PMTs on even strings, 64 on odd ones) with another collection efficiency"""
    functions, types, pmts, modules = PS.synthetic_layout()
    pmts = pmts.copy()
    pmts["collectionEfficiency"] = ce
    pmts["radius"] = radius_fraction * PS.RADIUS
    return functions, types, pmts, modules


def keep_all_layout(n_pmts=(31, 64), radius_fraction=0.2):
    """a layout under which a record of weight 1 that meets a PMT from the front has P = 1 exactly and is kept whatever the draw:
    G = Q = 1, ce = 1, A(c) = c on a two-point table (so A(c) / c = 1 -- c / c -- for every c in (0, 1]).  Discs of 0.2 R do not
    overlap as seen from the front, at 31 or at 64 PMTs"""
    functions = [PC.constant(1.0), PC.constant(1.0), PC.table(0.0, 1.0, [0.0, 1.0])]
    types = np.zeros(len(n_pmts), dtype=CV.PMT_TYPE_DTYPE)
    pmts = np.zeros(sum(n_pmts), dtype=CV.PMT_DTYPE)
    first = 0
    for t, n in enumerate(n_pmts):
        types[t] = (PS.RADIUS, first, n, 0, 0)
        axes = PC.fibonacci_axes(n)
        block = pmts[first:first + n]
        block["axis"], block["position"], block["radius"] = axes, 0.85 * PS.RADIUS * axes, radius_fraction * PS.RADIUS
        block["collectionEfficiency"], block["quantumEfficiency"], block["angularAcceptance"] = 1.0, 1, 2
        first += n
    modules = PS.synthetic_layout()[3].copy()
    modules["type"] = modules["stringID"] % len(n_pmts)
    return functions, types, pmts, modules


def write_input(path, records, series, functions, types, pmts, modules, seed=SEED):
    """the generator's description and the input as tests/pmt_photon_hits_host_main.cpp and
    clsim_amd/cxx/pmt_photon_hits_adapter_test.cxx read them"""
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", len(functions), len(types), len(pmts), len(modules), len(records), len(series), seed, 0))
        for fn in functions:
            if fn[0] == "table":
                f.write(struct.pack("<2q3d", 0, len(fn[3]), fn[1], fn[2], 0.0))
                f.write(np.asarray(fn[3], dtype="<f8").tobytes())
            else:
                f.write(struct.pack("<2q3d", 1, 0, 0.0, 0.0, fn[1]))
        for array, dtype in ((types, CV.PMT_TYPE_DTYPE), (pmts, CV.PMT_DTYPE), (modules, CV.PMT_MODULE_DTYPE), (records, CV.FRAME_PHOTON_DTYPE),
                             (series, CV.MCPE_SERIES_DTYPE)):
            f.write(np.ascontiguousarray(array, dtype=dtype).tobytes())
