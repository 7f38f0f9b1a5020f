"""Shared by tests/test_pmt_series.py and tests/test_pmt_series_gpu.py: an independent numpy restatement of the PMT series
definition (include/clsimhip.h, "PMT series"), the synthetic generator and hits both test files use, and the properties of an
output."""
import numpy as np

from clsim_amd import converter as CV
from tests import mcpe_series_common as S
from tests import pmt_common as P

tkey_of = S.tkey_of
module_code = S.dom_code            # ascending in (string ID signed, OM ID)
particle_table = S.particle_table
mask_of = S.mask_of
SPECIAL_TIMES = S.SPECIAL_TIMES
SPECIAL_BITS = {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001}


def numpy_series(hits, types, modules, particles=None, masked=None):
    """(records, series, counters) of the definition: np.searchsorted for the module list and the table, np.lexsort on (identifier,
    tkey, pmt, module rank, frame).  types / modules: what the generator was made of (PMT_TYPE_DTYPE, PMT_MODULE_DTYPE)."""
    h = np.ascontiguousarray(hits, dtype=CV.PMT_HIT_DTYPE)
    types = np.asarray(types, dtype=CV.PMT_TYPE_DTYPE)
    modules = np.asarray(modules, dtype=CV.PMT_MODULE_DTYPE)
    counters = dict.fromkeys(CV.PMT_SERIES_COUNTERS, 0)
    codes = module_code(modules["stringID"], modules["omID"])
    by_rank = np.argsort(codes, kind="stable")
    ranked = codes[by_rank]
    n_pmts = types["numPMTs"][modules["type"][by_rank]].astype(np.int64) if len(modules) else np.zeros(0, dtype=np.int64)
    code = module_code(h["stringID"], h["omID"])
    rank = np.searchsorted(ranked, code)
    inside = np.minimum(rank, max(len(ranked) - 1, 0))
    known = ((rank < len(ranked)) & (ranked[inside] == code)) if len(ranked) else np.zeros(len(h), dtype=bool)
    known &= (h["pmt"].astype(np.int64) < n_pmts[inside]) if len(ranked) else False
    counters["unknown_channel"] = int((~known).sum())
    if particles is None:
        frame = np.zeros(len(h), dtype=np.uint32)
        shift = np.zeros(len(h))
        found = np.ones(len(h), dtype=bool)
    else:
        p = np.ascontiguousarray(particles, dtype=CV.MCPE_PARTICLE_DTYPE)
        at = np.searchsorted(p["id"], h["id"])
        slot = np.minimum(at, max(len(p) - 1, 0))
        found = ((at < len(p)) & (p["id"][slot] == h["id"])) if len(p) else np.zeros(len(h), dtype=bool)
        frame = p["frame"][slot] if len(p) else np.zeros(len(h), dtype=np.uint32)
        shift = p["timeShift"][slot] if len(p) else np.zeros(len(h))
    counters["unknown_particle"] = int((known & ~found).sum())
    alive = known & found
    hidden = np.zeros(len(h), dtype=bool)
    if masked is not None and len(masked):
        k = np.ascontiguousarray(masked, dtype=CV.MCPE_MASK_DTYPE)
        hidden = np.isin(frame.astype(np.int64) * 2 ** 32 + code, k["frame"].astype(np.int64) * 2 ** 32 + module_code(k["stringID"], k["omID"]))
    counters["masked"] = int((alive & hidden).sum())
    alive &= ~hidden
    time = h["time"] + shift                          # one binary64 addition
    ident, frame, rank, pmt, time = h["id"][alive], frame[alive], rank[alive], h["pmt"][alive], time[alive]
    sid, oid = h["stringID"][alive], h["omID"][alive]
    order = np.lexsort((ident, tkey_of(time), pmt, rank, frame))
    out = np.zeros(len(order), dtype=CV.PMT_HIT_DTYPE)
    out["id"], out["stringID"], out["omID"], out["pmt"], out["time"] = ident[order], sid[order], oid[order], pmt[order], time[order]
    frame, rank, pmt = frame[order], rank[order], pmt[order]
    head = np.ones(len(out), dtype=bool)
    head[1:] = (frame[1:] != frame[:-1]) | (rank[1:] != rank[:-1]) | (pmt[1:] != pmt[:-1])
    first = np.flatnonzero(head)
    series = np.zeros(len(first), dtype=CV.PMT_SERIES_DTYPE)
    series["frame"], series["stringID"], series["omID"], series["pmt"] = frame[first], out["stringID"][first], out["omID"][first], pmt[first]
    series["first"] = first
    series["count"] = np.diff(np.append(first, len(out)))
    return out, series, counters


def check_properties(records, series):
    """the entries partition the records; the table is strictly ascending in (frame, string, om, pmt); inside a series the key
    (tkey, identifier) does not descend; reserved words are 0"""
    assert int(series["count"].sum()) == len(records)
    assert np.array_equal(series["first"], np.cumsum(series["count"].astype(np.int64)) - series["count"])
    assert (series["count"] > 0).all() and (series["reserved"] == 0).all() and (records["reserved"] == 0).all()
    module = series["frame"].astype(np.int64) * 2 ** 32 + module_code(series["stringID"], series["omID"])
    assert (np.diff(module) >= 0).all()
    same_module = np.diff(module) == 0
    assert (np.diff(series["pmt"].astype(np.int64))[same_module] > 0).all()
    owner = np.repeat(np.arange(len(series)), series["count"])
    assert np.array_equal(records["stringID"], series["stringID"][owner]) and np.array_equal(records["omID"], series["omID"][owner])
    assert np.array_equal(records["pmt"], series["pmt"][owner])
    t = tkey_of(records["time"])
    inner = owner[1:] == owner[:-1]
    assert (t[1:][inner] >= t[:-1][inner]).all()
    tie = inner & (t[1:] == t[:-1])
    assert (records["id"][1:][tie] >= records["id"][:-1][tie]).all()


# ---- synthetic inputs ----
# two types with different PMT counts, by string parity: the channel bases are a real prefix sum, and pmt = 63 occurs
PMT_COUNTS = (31, 64)
MODULE_STRINGS = np.repeat(np.array([-3, -1, 0, 1, 2, 40, 86], dtype=np.int32), 12)
MODULE_OMS = np.tile(np.arange(1, 13, dtype=np.uint32) * 5, 7)
RADIUS = 0.1651


def synthetic_layout():
    """(functions, types, pmts, modules): type 0 with 31 PMTs on even strings, type 1 with 64 on odd ones"""
    types = np.zeros(len(PMT_COUNTS), dtype=CV.PMT_TYPE_DTYPE)
    pmts = np.zeros(sum(PMT_COUNTS), dtype=CV.PMT_DTYPE)
    first = 0
    for t, n in enumerate(PMT_COUNTS):
        types[t] = (RADIUS, first, n, 0, 0)
        axes = P.fibonacci_axes(n)
        block = pmts[first:first + n]
        block["axis"], block["position"], block["radius"] = axes, 0.85 * RADIUS * axes, 0.2 * RADIUS
        block["collectionEfficiency"], block["quantumEfficiency"], block["angularAcceptance"] = 0.9, 1, 2
        first += n
    modules = np.zeros(len(MODULE_STRINGS), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"] = MODULE_STRINGS, MODULE_OMS
    modules["type"] = MODULE_STRINGS % 2
    modules["rotation"] = np.eye(3).reshape(9)
    # (given in another order than the ranks': the generator must sort them itself)
    modules = modules[np.random.default_rng(99).permutation(len(modules))]
    return P.standard_functions(), types, pmts, modules


def synthetic_generator():
    functions, types, pmts, modules = synthetic_layout()
    return P.make_generator(functions, types, pmts, modules), types, modules


def synthetic_hits(n, seed, n_identifiers=40, first_identifier=1000, special=True, ties=True):
    """n hits at the synthetic generator's modules, every PMT number of the module's type: identifiers first ... first +
    n_identifiers - 1, times around 1 us, a share of exactly equal times under different identifiers, and the special values"""
    rng = np.random.default_rng(seed)
    h = np.zeros(n, dtype=CV.PMT_HIT_DTYPE)
    module = rng.integers(0, len(MODULE_STRINGS), n)
    h["stringID"], h["omID"] = MODULE_STRINGS[module], MODULE_OMS[module]
    h["pmt"] = rng.integers(0, 1 << 30, n) % np.asarray(PMT_COUNTS)[MODULE_STRINGS[module] % 2]
    h["id"] = first_identifier + rng.integers(0, n_identifiers, n)
    h["time"] = rng.uniform(500.0, 4000.0, n)
    if ties and n >= 8:
        h["time"][: n // 4] = np.round(h["time"][: n // 4])       # whole nanoseconds: many equal times
        # ... and an eighth of the hits on four PMTs at five times: equal time' under different identifiers in one series
        crowd = slice(n // 4, n // 4 + n // 8)
        k = rng.integers(0, 4, n // 8)
        h["stringID"][crowd], h["omID"][crowd] = np.array([-1, 0, 1, 86])[k], np.array([10, 20, 25, 60])[k]
        h["pmt"][crowd] = np.array([7, 30, 63, 0])[k]
        h["time"][crowd] = 1000.0 + 250.0 * rng.integers(0, 5, n // 8)
    if special and n >= 4 * len(SPECIAL_TIMES):
        at = rng.choice(n, 4 * len(SPECIAL_TIMES), replace=False)
        h["time"][at] = np.tile(SPECIAL_TIMES, 4)
        h["pmt"][at[:4]] = (63, 63, 30, 0)
        h["stringID"][at[:4]], h["omID"][at[:4]] = (-3, 1, 2, 40), (5, 60, 5, 30)
    return h


def one_channel_hits(n, seed, string_id=1, om_id=25, pmt=63, n_identifiers=40):
    """n hits in one (module, PMT)"""
    h = synthetic_hits(n, seed, n_identifiers=n_identifiers, special=False)
    h["stringID"], h["omID"], h["pmt"] = string_id, om_id, pmt
    return h


def same(got, want):
    """records, series and counters, arrays as they are"""
    assert got[2] == want[2]
    assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()
    assert got[1].dtype == want[1].dtype and got[1].tobytes() == want[1].tobytes()
