"""Shared by tests/test_mcpe_merge.py and tests/test_mcpe_merge_gpu.py: an independent numpy restatement of the MCPE merging
definition (include/clsimhip.h, "MCPE merging"), the properties the definition promises, and the small inputs both files use."""
import math
from fractions import Fraction

import numpy as np

from clsim_amd import converter as CV
from tests import mcpe_series_common as S


def numpy_merge(records, series, window):
    """(merged, merged_series, parents, ranges) of the definition: a plain Python loop per series in binary64 (Python floats),
    np.unique for the parents"""
    records = np.ascontiguousarray(records, dtype=CV.MCPE_DTYPE)
    series = np.ascontiguousarray(series, dtype=CV.MCPE_SERIES_DTYPE)
    window = float(window)
    merged, parents = [], []
    out_series = series.copy()
    ranges = np.zeros(len(series), dtype=CV.MCPE_PARENT_RANGE_DTYPE)
    n_merged = n_parents = 0
    for k in range(len(series)):
        first, count = int(series["first"][k]), int(series["count"][k])
        times = records["time"][first:first + count].tolist()
        group = np.zeros(count, dtype=np.uint64)
        openers, T, g = [], None, -1
        for j, t in enumerate(times):
            if j == 0 or not math.isfinite(t) or not math.isfinite(T) or t - T > window:
                g += 1
                T = t
                openers.append(j)
            group[j] = g
        part = np.zeros(len(openers), dtype=CV.MCPE_MERGED_DTYPE)
        at = first + np.asarray(openers, dtype=np.int64)
        part["npe"] = np.diff(np.append(openers, count))
        part["stringID"], part["omID"], part["time"] = records["stringID"][at], records["omID"][at], records["time"][at]
        merged.append(part)
        pairs = np.unique((records["id"][first:first + count].astype(np.uint64) << np.uint64(32)) | group)
        p = np.zeros(len(pairs), dtype=CV.MCPE_PARENT_DTYPE)
        p["id"], p["index"] = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
        parents.append(p)
        out_series["first"][k], out_series["count"][k] = n_merged, len(part)
        ranges["first"][k], ranges["count"][k] = n_parents, len(p)
        n_merged += len(part)
        n_parents += len(p)
    merged = np.concatenate(merged) if merged else np.zeros(0, dtype=CV.MCPE_MERGED_DTYPE)
    parents = np.concatenate(parents) if parents else np.zeros(0, dtype=CV.MCPE_PARENT_DTYPE)
    return merged, out_series, parents, ranges


def same(got, want):
    """the four arrays as they are"""
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and len(g) == len(w)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    assert len(got) == len(want) == 4


def check_properties(records, series, window, out):
    """what the definition promises, from the arrays alone"""
    merged, merged_series, parents, ranges = out
    window = float(window)
    assert int(merged["npe"].astype(np.int64).sum()) == len(records) and (merged["npe"] >= 1).all()
    # the merged table: the same entries in the same order, partitioning the merged records
    for name in ("frame", "stringID", "omID"):
        assert np.array_equal(merged_series[name], series[name])
    assert len(merged_series) == len(series) == len(ranges)
    for table, total in ((merged_series, len(merged)), (ranges, len(parents))):
        assert int(table["count"].astype(np.int64).sum()) == total and (table["count"] > 0).all()
        assert np.array_equal(table["first"], (np.cumsum(table["count"].astype(np.int64)) - table["count"]).astype(np.uint32))
    owner = np.repeat(np.arange(len(series)), merged_series["count"])                    # series of every merged record
    assert np.array_equal(merged["stringID"], series["stringID"][owner]) and np.array_equal(merged["omID"], series["omID"][owner])
    # groups are consecutive records; the opener gives the time
    start = np.concatenate([[0], np.cumsum(merged["npe"].astype(np.int64))])
    assert np.array_equal(records["time"][start[:-1]].view(np.uint64), merged["time"].view(np.uint64))
    assert np.array_equal(start[:-1][merged_series["first"]], series["first"])          # groups never span series
    t = records["time"]
    last = t[start[1:] - 1]
    finite_opener = np.isfinite(merged["time"])
    with np.errstate(over="ignore", invalid="ignore"):
        # every group spans at most window; a group behind an opener that is not finite is that record alone
        assert not ((last - merged["time"])[finite_opener] > window).any()
        assert (merged["npe"][~finite_opener] == 1).all()
        assert np.isfinite(t[np.repeat(finite_opener, merged["npe"])]).all()
        # consecutive finite openers of a series differ by more than window
        both = (owner[1:] == owner[:-1]) & finite_opener[1:] & finite_opener[:-1]
        assert ((merged["time"][1:] - merged["time"][:-1])[both] > window).all()
        # fl(t - T) is monotone in t: behind every finite opener, over the finite rest of its series
        group_of = np.repeat(np.arange(len(merged)), merged["npe"])
        series_of = np.repeat(np.arange(len(series)), series["count"])
        for g in np.flatnonzero(finite_opener)[:: max(1, len(merged) // 200)]:
            rest = t[start[g]: series["first"][owner[g]] + series["count"][owner[g]]]
            rest = rest[np.isfinite(rest)]
            assert (np.diff(rest - merged["time"][g]) >= 0).all()
    # the parents: the distinct (series, identifier, group within the series), ascending
    index = group_of - merged_series["first"][series_of]
    want = np.unique(np.stack([series_of.astype(np.uint64), records["id"].astype(np.uint64), index.astype(np.uint64)], axis=1), axis=0) \
        if len(records) else np.zeros((0, 3), dtype=np.uint64)
    got = np.stack([np.repeat(np.arange(len(series)), ranges["count"]).astype(np.uint64), parents["id"].astype(np.uint64),
                    parents["index"].astype(np.uint64)], axis=1)
    assert np.array_equal(got, want)


# ---- inputs ----
def mcpes_of(entries):
    """[(identifier, DOM number among the synthetic generator's, time)] -> MCPE_DTYPE, in the order given"""
    m = np.zeros(len(entries), dtype=CV.MCPE_DTYPE)
    for i, (ident, dom, time) in enumerate(entries):
        m[i] = (ident, S.DOM_STRINGS[dom], S.DOM_OMS[dom], time)
    return m


def series_of(gen, mcpes):
    """(records, series) of the series stage with one frame and a shift of -0.0, which keeps every bit pattern of the times"""
    p = S.particle_table(mcpes["id"] if len(mcpes) else [0], frames=(3,))
    p["timeShift"] = -0.0
    records, series, counters = gen.MakeSeriesHost(mcpes, p)
    assert not any(counters.values()) and len(records) == len(mcpes)
    return records, series


UP = float(np.nextafter(1002.0, np.inf))
BIG = 2.0 ** 53


def edge_cases():
    """name -> (entries, window, npe of the merged records in order, parents in order or None)"""
    cases = {}
    # window = 0: only bit-equal finite times merge, and -0.0 and +0.0 merge
    cases["window_zero"] = ([(4, 0, 5.0), (2, 0, 0.0), (1, 0, float(np.nextafter(5.0, np.inf))), (3, 0, 5.0), (9, 0, -0.0), (8, 0, 5.0)], 0.0, [2, 3, 1],
                            [(1, 2), (2, 0), (3, 1), (4, 1), (8, 1), (9, 0)])
    # exactly window apart joins, one ulp further opens
    cases["exactly_window"] = ([(1, 1, 1000.0), (2, 1, 1002.0), (3, 1, UP)], 2.0, [2, 1], [(1, 0), (2, 0), (3, 1)])
    # the real difference 2^53 + 1 exceeds the window 2^53, the rounded difference equals it: joins
    cases["rounded_difference"] = ([(1, 2, -1.0), (2, 2, BIG)], BIG, [2], [(1, 0), (2, 0)])
    # a difference that overflows to +inf opens
    cases["overflow"] = ([(1, 3, -1e308), (2, 3, 1.7e308)], 1e308, [1, 1], [(1, 0), (2, 1)])
    # one particle in many groups; many particles in one group; a series of one record beside them
    cases["one_particle_many_groups"] = ([(7, 4, 10.0 * k) for k in range(40)] + [(7, 5, 3.0)], 1.0, [1] * 41, [(7, k) for k in range(40)] + [(7, 0)])
    cases["many_particles_one_group"] = ([(100 + (37 * k) % 90, 6, 50.0 + 0.01 * k) for k in range(90)], 1.0, [90], [(100 + k, 0) for k in range(90)])
    # the same identifier twice in one group at different times, with other identifiers between them: one parent entry
    cases["identifier_twice"] = ([(5, 7, 0.0), (9, 7, 0.1), (3, 7, 0.2), (5, 7, 0.3), (5, 7, 9.0)], 1.0, [4, 1], [(3, 0), (5, 0), (5, 1), (9, 0)])
    cases["one_record"] = ([(1, 8, 1.5)], 10.0, [1], [(1, 0)])
    cases["no_record"] = ([], 10.0, [], [])
    # every special bit pattern is a group of its own, twice each under different identifiers; the finite ones between them
    special = [(10 + k, 9, float(t)) for k, t in enumerate(np.tile(S.SPECIAL_TIMES, 2))]
    cases["special_times"] = (special, 3e300, None, None)
    return cases


def check_edge_claims():
    """the inputs are what their names say"""
    assert Fraction(BIG) - Fraction(-1.0) > Fraction(BIG) and BIG - (-1.0) == BIG
    assert 1002.0 - 1000.0 == 2.0 and UP - 1000.0 > 2.0
    assert 1.7e308 - (-1e308) == math.inf
    bits = set(np.asarray(S.SPECIAL_TIMES).view(np.uint64).tolist())
    assert {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001} <= bits


def sized_series(counts, seed, span=3000.0, n_identifiers=9):
    """one DOM per entry of `counts` with that many records at random times in [0, span)"""
    rng = np.random.default_rng(seed)
    m = np.zeros(int(sum(counts)), dtype=CV.MCPE_DTYPE)
    at = 0
    for dom, c in enumerate(counts):
        m["stringID"][at:at + c], m["omID"][at:at + c] = S.DOM_STRINGS[dom], S.DOM_OMS[dom]
        at += c
    m["time"] = rng.uniform(0.0, span, len(m))
    m["id"] = 500 + rng.integers(0, n_identifiers, len(m))
    return m[rng.permutation(len(m))]


def one_dom(n, seed, n_identifiers=7):
    """n records of n_identifiers particles at one DOM, times in [0, 1e6)"""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=CV.MCPE_DTYPE)
    m["stringID"], m["omID"] = -1, 25
    m["time"] = rng.uniform(0.0, 1e6, n)
    m["id"] = 1000 + rng.integers(0, n_identifiers, n)
    return m
