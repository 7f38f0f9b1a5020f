"""Shared by tests/test_frame_photons.py and tests/test_frame_photons_gpu.py: an independent numpy restatement of the frame photons
definition (include/clsimhip.h, "Frame photons") -- np.lexsort on the full order, h included -- and the synthetic inputs both test
files use."""
import functools

import numpy as np

from clsim_amd import converter as CV
from tests import mcpe_series_common as S

U32 = np.uint32
FLOATS = ("weight", "wavelength", "groupVelocity", "x", "y", "z", "theta", "phi")        # w0 ... w7, in declared order
BOUND = 2048
tkey_of = S.tkey_of
dom_code = S.dom_code
particle_table = S.particle_table
mask_of = S.mask_of
DOM_STRINGS, DOM_OMS = S.DOM_STRINGS, S.DOM_OMS


def words_of(records):
    """(n, 8) uint32: the eight float fields' bit patterns, of photons or of output records"""
    return np.stack([np.ascontiguousarray(records[name]).view(U32) for name in FLOATS], axis=1)


def mix(words):
    """h: FNV-1a over the 32 bytes of w0 ... w7, each word least significant byte first"""
    words = np.asarray(words, dtype=U32).reshape(-1, 8)
    h = np.full(len(words), 2166136261, dtype=np.uint64)
    for k in range(8):
        for b in range(4):
            h ^= (words[:, k].astype(np.uint64) >> np.uint64(8 * b)) & np.uint64(255)
            h = (h * np.uint64(16777619)) & np.uint64(0xFFFFFFFF)
    return h.astype(U32)


def numpy_frame_photons(photons, dom_strings, dom_oms, particles=None, masked=None):
    """(records, series, counters) of the definition"""
    m = np.ascontiguousarray(photons, dtype=CV.PHOTON_DTYPE)
    counters = dict.fromkeys(CV.FRAME_PHOTON_COUNTERS, 0)
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
        hidden = np.isin(frame.astype(np.int64) * 2 ** 32 + code, k["frame"].astype(np.int64) * 2 ** 32 + dom_code(k["stringID"], k["omID"]))
    counters["masked"] = int((alive & hidden).sum())
    alive &= ~hidden
    with np.errstate(invalid="ignore"):
        time = m["t"].astype(np.float64) + shift        # widened, then one binary64 addition
    m, frame, rank, time = m[alive], frame[alive], rank[alive], time[alive]
    w = words_of(m)
    h = mix(w)
    t = tkey_of(time)
    order = np.lexsort(tuple(w[:, k] for k in range(7, -1, -1)) + (h, m["id"], t, rank, frame))
    m, frame, rank, time, w, h, t = m[order], frame[order], rank[order], time[order], w[order], h[order], t[order]
    # the bound: runs equal in (frame, module, tkey, identifier, h) with two distinct contents (sorted: first and last differ)
    new_run = np.ones(len(m), dtype=bool)
    new_run[1:] = (frame[1:] != frame[:-1]) | (rank[1:] != rank[:-1]) | (t[1:] != t[:-1]) | (m["id"][1:] != m["id"][:-1]) | (h[1:] != h[:-1])
    begin = np.flatnonzero(new_run)
    end = np.append(begin[1:], len(m))
    for b, e in zip(begin[end - begin > BOUND], end[end - begin > BOUND]):
        if (w[b] != w[e - 1]).any():
            counters["tie_overflow"] += int(e - b)
    if counters["tie_overflow"]:
        return np.zeros(0, dtype=CV.FRAME_PHOTON_DTYPE), np.zeros(0, dtype=CV.MCPE_SERIES_DTYPE), counters
    out = np.zeros(len(m), dtype=CV.FRAME_PHOTON_DTYPE)
    out["id"], out["stringID"], out["omID"], out["time"] = m["id"], m["stringID"], m["omID"], time
    for name in FLOATS:
        out[name] = m[name]
    head = np.ones(len(out), dtype=bool)
    head[1:] = (frame[1:] != frame[:-1]) | (rank[1:] != rank[:-1])
    first = np.flatnonzero(head)
    series = np.zeros(len(first), dtype=CV.MCPE_SERIES_DTYPE)
    series["frame"], series["stringID"], series["omID"], series["first"] = frame[first], out["stringID"][first], out["omID"][first], first
    series["count"] = np.diff(np.append(first, len(out)))
    return out, series, counters


def check_properties(records, series):
    """from the arrays alone: the series partition the records; frames and modules ascend strictly; within a series the order is
    (tkey, identifier, h, w0 ... w7), non-decreasing, and equal neighbours are byte-identical"""
    assert int(series["count"].sum()) == len(records)
    if len(records) == 0:
        assert len(series) == 0
        return
    assert np.array_equal(series["first"], np.concatenate([[0], np.cumsum(series["count"].astype(np.int64))[:-1]]).astype(np.uint32))
    assert (series["count"] > 0).all()
    key = series["frame"].astype(np.int64) * 2 ** 32 + dom_code(series["stringID"], series["omID"])
    assert (np.diff(key) > 0).all()
    owner = np.repeat(np.arange(len(series)), series["count"])
    assert np.array_equal(records["stringID"], series["stringID"][owner]) and np.array_equal(records["omID"], series["omID"][owner])
    w = words_of(records)
    columns = [tkey_of(records["time"]), records["id"].astype(np.uint64), mix(w).astype(np.uint64)] + [w[:, k].astype(np.uint64) for k in range(8)]
    inner = owner[1:] == owner[:-1]
    undecided = inner.copy()            # neighbours of one series that are equal in every column so far
    for c in columns:
        assert not (undecided & (c[1:] < c[:-1])).any()
        undecided &= c[1:] == c[:-1]
    raw = records.view(np.uint8).reshape(len(records), -1)
    assert (raw[1:][undecided] == raw[:-1][undecided]).all()


def same(got, want):
    for g, w in zip(got[:2], want[:2]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert got[2] == want[2]


# ---- synthetic inputs ----
def synthetic_doms():
    return CV.FramePhotonDoms(DOM_STRINGS, DOM_OMS)


SPECIAL_TIMES = np.array([0.0, -0.0, np.inf, -np.inf, 0.0, 0.0, 1.0, -1.0, 1e-45, -1e-45, 3e38, -3e38], dtype=np.float32)
SPECIAL_TIMES.view(U32)[4] = 0x7FC00000        # a positive NaN
SPECIAL_TIMES.view(U32)[5] = 0xFFC00001        # a negative NaN, with a payload


def synthetic_photons(n, seed, n_identifiers=40, first_identifier=1000, special=True, quantised=True):
    """n photon records at the synthetic DOMs.  quantised: a quarter of them at a handful of modules, whole-microsecond times and few
    identifiers, with differing contents -- ties in (frame, module, tkey, identifier) that only h and the words decide -- and
    some exact copies among them"""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=CV.PHOTON_DTYPE)
    dom = rng.integers(0, len(DOM_STRINGS), n)
    m["stringID"], m["omID"] = DOM_STRINGS[dom], DOM_OMS[dom]
    m["id"] = first_identifier + rng.integers(0, n_identifiers, n)
    m["t"] = rng.uniform(500.0, 4000.0, n)
    for name in ("x", "y", "z", "sx", "sy", "sz"):
        m[name] = rng.uniform(-500.0, 500.0, n)
    for name in ("theta", "stheta"):
        m[name] = rng.uniform(0.0, np.pi, n)
    for name in ("phi", "sphi"):
        m[name] = rng.uniform(0.0, 2 * np.pi, n)
    m["wavelength"] = rng.uniform(2.6e-7, 6.9e-7, n)
    m["cherenkovDist"], m["distInAbsLens"], m["st"] = rng.uniform(0.0, 300.0, n), rng.uniform(0.0, 5.0, n), rng.uniform(0.0, 400.0, n)
    m["numScatters"] = rng.integers(0, 50, n)
    m["weight"] = rng.uniform(0.5, 2.0, n)
    m["groupVelocity"] = rng.uniform(0.21, 0.23, n)
    if quantised and n >= 8:
        q = n // 4
        m["t"][:q] = 1000.0 * rng.integers(1, 4, q)
        d = rng.integers(0, 3, q)
        m["stringID"][:q], m["omID"][:q] = DOM_STRINGS[d], DOM_OMS[d]
        m["id"][:q] = first_identifier + rng.integers(0, 2, q)
        m[q // 2:q] = m[rng.integers(0, max(q // 2, 1), q - q // 2)]        # exact copies of some of them
    if special and n >= 4 * len(SPECIAL_TIMES):
        at = n // 4 + rng.choice(n - n // 4, 4 * len(SPECIAL_TIMES), replace=False)
        m["t"][at] = np.tile(SPECIAL_TIMES, 4)
    return m


def content_ties(records):
    """neighbours of the output equal in (frame's series, tkey, identifier) whose contents differ"""
    t = tkey_of(records["time"])
    w = words_of(records)
    return int(((records["stringID"][1:] == records["stringID"][:-1]) & (records["omID"][1:] == records["omID"][:-1]) & (t[1:] == t[:-1]) &
                (records["id"][1:] == records["id"][:-1]) & (w[1:] != w[:-1]).any(axis=1)).sum())


@functools.lru_cache(maxsize=None)
def colliding_pair(seed=5, tries=300000):
    """two distinct payloads (8 words each) with the same h, by birthday search over `tries` random payloads (about tries^2 / 2^33 = 10
    pairs are expected); fails loudly when there is none"""
    rng = np.random.default_rng(seed)
    floats = np.stack([rng.uniform(0.5, 2.0, tries), rng.uniform(2.6e-7, 6.9e-7, tries), rng.uniform(0.21, 0.23, tries), rng.uniform(-500, 500, tries),
                       rng.uniform(-500, 500, tries), rng.uniform(-500, 500, tries), rng.uniform(0, np.pi, tries), rng.uniform(0, 2 * np.pi, tries)],
                      axis=1).astype(np.float32)
    words = floats.view(U32)
    h = mix(words)
    order = np.argsort(h, kind="stable")
    hit = np.flatnonzero((h[order][1:] == h[order][:-1]) & (words[order][1:] != words[order][:-1]).any(axis=1))
    assert len(hit) > 0, "no collision of h among %d random payloads: the search, or h, is not what it is meant to be" % tries
    a, b = words[order[hit[0]]], words[order[hit[0] + 1]]
    assert mix(a)[0] == mix(b)[0] and (a != b).any()
    return a.copy(), b.copy()


def collision_run(length, seed, only_a=False):
    """`length` photons at one module, time and particle with the payloads of colliding_pair(), mixed in shuffled positions, among
    200 ordinary photons"""
    a, b = colliding_pair()
    rng = np.random.default_rng(seed)
    run = np.zeros(length, dtype=CV.PHOTON_DTYPE)
    run["stringID"], run["omID"], run["id"], run["t"] = 1, 25, 1003, 1234.5
    which = np.zeros(length, dtype=bool) if only_a else rng.integers(0, 2, length).astype(bool)
    if not only_a and length >= 2:
        which[0], which[-1] = False, True
    for k, name in enumerate(FLOATS):
        run[name] = np.where(which, b[k], a[k]).astype(U32).view(np.float32)
    run["numScatters"] = rng.integers(0, 9, length)         # (not part of the output: records with equal payloads stay equal)
    m = np.concatenate([synthetic_photons(200, seed + 1, special=False), run])
    return m[rng.permutation(len(m))]
