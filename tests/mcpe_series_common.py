"""Shared by tests/test_mcpe_series.py and tests/test_mcpe_series_gpu.py: an independent numpy restatement of the MCPE series
definition (include/clsimhip.h, "MCPE series") and the synthetic inputs both test files use."""
import numpy as np

from clsim_amd import converter as CV
from tests import mcpe_common as M

U64 = np.uint64


def tkey_of(times):
    """the order-preserving 64-bit image of a binary64: b ^ (b >> 63 ? ~0 : 1 << 63)"""
    b = np.ascontiguousarray(times, dtype=np.float64).view(np.uint64)
    return np.where((b >> U64(63)) != 0, ~b, b | (U64(1) << U64(63)))


def dom_code(string_ids, om_ids):
    """ascending in (string ID signed, OM ID)"""
    return (np.asarray(string_ids).astype(np.int64) + 32768) * 65536 + np.asarray(om_ids).astype(np.int64)


def numpy_series(mcpes, dom_strings, dom_oms, particles=None, masked=None):
    """(records, series, counters) of the definition: np.searchsorted for the table, np.lexsort on (identifier, tkey, DOM rank,
    frame).  dom_strings / dom_oms: the generator's DOM list."""
    m = np.ascontiguousarray(mcpes, dtype=CV.MCPE_DTYPE)
    counters = dict.fromkeys(CV.MCPE_SERIES_COUNTERS, 0)
    doms = np.unique(dom_code(dom_strings, dom_oms))
    code = dom_code(m["stringID"], m["omID"])
    rank = np.searchsorted(doms, code)
    known = (rank < len(doms)) & (doms[np.minimum(rank, max(len(doms) - 1, 0))] == code) if len(doms) else np.zeros(len(m), dtype=bool)
    counters["unknown_dom"] = int((~known).sum())
    if particles is None:
        frame = np.zeros(len(m), dtype=np.uint32)
        shift = np.zeros(len(m))
        found = np.ones(len(m), dtype=bool)
    else:
        p = np.ascontiguousarray(particles, dtype=CV.MCPE_PARTICLE_DTYPE)
        at = np.searchsorted(p["id"], m["id"])
        inside = np.minimum(at, max(len(p) - 1, 0))
        found = (at < len(p)) & (p["id"][inside] == m["id"]) if len(p) else np.zeros(len(m), dtype=bool)
        frame = p["frame"][inside] if len(p) else np.zeros(len(m), dtype=np.uint32)
        shift = p["timeShift"][inside] if len(p) else np.zeros(len(m))
    counters["unknown_particle"] = int((known & ~found).sum())
    alive = known & found
    hidden = np.zeros(len(m), dtype=bool)
    if masked is not None and len(masked):
        k = np.ascontiguousarray(masked, dtype=CV.MCPE_MASK_DTYPE)
        mask_code = k["frame"].astype(np.int64) * 2 ** 32 + dom_code(k["stringID"], k["omID"])
        hidden = np.isin(frame.astype(np.int64) * 2 ** 32 + code, mask_code)
    counters["masked"] = int((alive & hidden).sum())
    alive &= ~hidden
    time = m["time"] + shift                          # one binary64 addition
    ident, frame, rank, time, sid, oid = m["id"][alive], frame[alive], rank[alive], time[alive], m["stringID"][alive], m["omID"][alive]
    order = np.lexsort((ident, tkey_of(time), rank, frame))
    out = np.zeros(len(order), dtype=CV.MCPE_DTYPE)
    out["id"], out["stringID"], out["omID"], out["time"] = ident[order], sid[order], oid[order], time[order]
    frame, rank = frame[order], rank[order]
    head = np.ones(len(out), dtype=bool)
    head[1:] = (frame[1:] != frame[:-1]) | (rank[1:] != rank[:-1])
    first = np.flatnonzero(head)
    series = np.zeros(len(first), dtype=CV.MCPE_SERIES_DTYPE)
    series["frame"], series["stringID"], series["omID"], series["first"] = frame[first], out["stringID"][first], out["omID"][first], first
    series["count"] = np.diff(np.append(first, len(out)))
    return out, series, counters


def check_properties(records, series):
    """series partition the records; strictly ascending in (frame, string, om); tkey non-decreasing inside a series"""
    assert int(series["count"].sum()) == len(records)
    assert np.array_equal(series["first"], np.concatenate([[0], np.cumsum(series["count"].astype(np.int64))[:-1]]).astype(np.uint32))
    assert (series["count"] > 0).all()
    key = series["frame"].astype(np.int64) * 2 ** 32 + dom_code(series["stringID"], series["omID"])
    assert (np.diff(key) > 0).all()
    owner = np.repeat(np.arange(len(series)), series["count"])
    assert np.array_equal(records["stringID"], series["stringID"][owner]) and np.array_equal(records["omID"], series["omID"][owner])
    t = tkey_of(records["time"])
    inner = owner[1:] == owner[:-1]
    assert (t[1:][inner] >= t[:-1][inner]).all()


# ---- synthetic inputs ----
DOM_STRINGS = np.repeat(np.array([-3, -1, 0, 1, 2, 40, 86], dtype=np.int32), 12)
DOM_OMS = np.tile(np.arange(1, 13, dtype=np.uint32) * 5, 7)


def synthetic_generator():
    return M.make_generator([M.acceptance_table()], DOM_STRINGS, DOM_OMS, np.zeros(len(DOM_STRINGS), dtype=np.int32))


SPECIAL_TIMES = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0, 5e-324, -5e-324, 1e300, -1e300], dtype=np.float64)
SPECIAL_TIMES[5] = np.frombuffer(np.uint64(0xFFF8000000000001).tobytes(), dtype=np.float64)[0]       # a negative NaN
SPECIAL_TIMES[4] = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), dtype=np.float64)[0]       # a positive NaN


def synthetic_mcpes(n, seed, n_identifiers=40, first_identifier=1000, special=True, ties=True):
    """n MCPEs at the synthetic generator's DOMs: identifiers first ... first + n_identifiers - 1, times around 1 us, a share of
    exactly equal times under different identifiers, and the special values"""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=CV.MCPE_DTYPE)
    dom = rng.integers(0, len(DOM_STRINGS), n)
    m["stringID"], m["omID"] = DOM_STRINGS[dom], DOM_OMS[dom]
    m["id"] = first_identifier + rng.integers(0, n_identifiers, n)
    m["time"] = rng.uniform(500.0, 4000.0, n)
    if ties and n >= 8:
        m["time"][: n // 4] = np.round(m["time"][: n // 4])       # whole nanoseconds: many equal times
    if special and n >= 4 * len(SPECIAL_TIMES):
        at = rng.choice(n, 4 * len(SPECIAL_TIMES), replace=False)
        m["time"][at] = np.tile(SPECIAL_TIMES, 4)
    return m


def particle_table(identifiers, frames=(7, 2, 900), shift_scale=100.0):
    """every identifier in ascending order; frames dealt round robin, so each frame's identifiers are interleaved with the others'"""
    ids = np.unique(np.asarray(identifiers, dtype=np.uint32))
    p = np.zeros(len(ids), dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"] = ids
    p["frame"] = np.asarray(frames, dtype=np.uint32)[np.arange(len(ids)) % len(frames)]
    p["timeShift"] = (np.arange(len(ids)) % 5 - 2) * shift_scale + 0.125
    return p


def mask_of(entries):
    k = np.zeros(len(entries), dtype=CV.MCPE_MASK_DTYPE)
    for i, (frame, s, o) in enumerate(entries):
        k[i] = (frame, s, o)
    return k
