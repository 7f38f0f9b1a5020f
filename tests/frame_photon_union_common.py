"""Shared by tests/test_frame_photon_union.py and tests/test_frame_photon_union_gpu.py: an independent numpy restatement of the union
and the split of the frame photon store (include/clsimhip.h, "Frame photon store") -- np.lexsort of the concatenation over the 14
words of the key, the table from the heads --, the synthetic inputs both test files use, and one crafted input per rule of the
series form."""
import numpy as np

from clsim_amd import converter as CV
from tests import frame_photons_common as F

FRAMES = (50, 10, 40, 20, 30)
MASK = F.mask_of([(10, 1, 10), (50, -3, 60), (30, 86, 30)])
SIZES = [(0, 0), (0, 100), (100, 0), (63, 65), (2049, 6145), (20000, 300)]
ALL = 0xFFFFFFFF
# NaN times of both signs, quiet and signalling, with payloads; the union moves them as bit patterns
NAN_TIME_BITS = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FF4000000000ABC, 0xFFF7FFFFFFFFFFFF,
                          0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)


def frames_of(series):
    return np.repeat(series["frame"], series["count"])


def table_of(records, frame):
    """the series table of records that ascend in (frame, DOM code, ...)"""
    code = F.dom_code(records["stringID"], records["omID"])
    head = np.ones(len(records), dtype=bool)
    head[1:] = (frame[1:] != frame[:-1]) | (code[1:] != code[:-1])
    first = np.flatnonzero(head)
    series = np.zeros(len(first), dtype=CV.MCPE_SERIES_DTYPE)
    series["frame"], series["stringID"], series["omID"], series["first"] = frame[first], records["stringID"][first], records["omID"][first], first
    series["count"] = np.diff(np.append(first, len(records)))
    return series


def key_order(records, frame):
    """np.lexsort over the 14 words: frame, DOM code, tkey (its two words as one integer), identifier, h, w0 ... w7"""
    w = F.words_of(records)
    return np.lexsort(tuple(w[:, k] for k in range(7, -1, -1)) + (F.mix(w), records["id"], F.tkey_of(records["time"]),
                                                                  F.dom_code(records["stringID"], records["omID"]), frame))


def numpy_union(a_records, a_series, b_records, b_series):
    records = np.concatenate([a_records, b_records])
    frame = np.concatenate([frames_of(a_series), frames_of(b_series)])
    order = key_order(records, frame)
    records, frame = records[order], frame[order]
    return records, table_of(records, frame)


def numpy_split(records, series, last_frame):
    head = series["frame"].astype(np.int64) <= last_frame
    assert not head[np.argmin(head):].any() if len(head) and not head.all() else True       # a prefix
    h = int(head.sum())
    n = int(series["count"][:h].sum())
    tail = series[h:].copy()
    tail["first"] -= n
    return records[:n], series[:h], records[n:], tail


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))


def particles():
    return F.particle_table(np.arange(1000, 1040), frames=FRAMES)


def bunch(n, seed, **kwargs):
    """n synthetic photons with the special times and content ties, whose identifiers the particle table deals to five frames"""
    return F.synthetic_photons(n, seed, **kwargs)


def frame_photons_of(doms, photons):
    records, series, counters = doms.MakeFramePhotonsHost(photons, particles(), MASK)
    assert counters["tie_overflow"] == 0 and counters["unknown_particle"] == 0 and counters["unknown_dom"] == 0
    return records, series


def pair(doms, n_a, n_b, seed=21):
    """the frame photons of the two parts of one bunch of n_a + n_b photons (the mask takes a few away), and of the whole"""
    m = bunch(n_a + n_b, seed)
    return frame_photons_of(doms, m[:n_a]), frame_photons_of(doms, m[n_a:]), frame_photons_of(doms, m)


def form_of(records, frames):
    """the series form of records with the frame of each given: np.lexsort on the key -- every record is kept"""
    records, frames = np.ascontiguousarray(records, dtype=CV.FRAME_PHOTON_DTYPE), np.asarray(frames, dtype=np.uint32)
    order = key_order(records, frames)
    return records[order], table_of(records[order], frames[order])


def records_of(photons):
    """frame photon records of photons as they are: no table, no mask, the time widened"""
    photons = np.ascontiguousarray(photons, dtype=CV.PHOTON_DTYPE)
    out = np.zeros(len(photons), dtype=CV.FRAME_PHOTON_DTYPE)
    out["id"], out["stringID"], out["omID"], out["time"] = photons["id"], photons["stringID"], photons["omID"], photons["t"].astype(np.float64)
    for name in F.FLOATS:
        out[name] = photons[name]
    return out


def exact_pair(n_a, n_b, seed=31):
    """two series forms of exactly n_a and n_b records over the same frames and modules, content ties and exact copies among them"""
    r = records_of(F.synthetic_photons(n_a + n_b, seed))
    frames = np.asarray(FRAMES, dtype=np.uint32)[r["id"] % len(FRAMES)]
    return form_of(r[:n_a], frames[:n_a]), form_of(r[n_a:], frames[n_a:])


def one_module(n, seed, **kwargs):
    """n records on one module in one frame: one series"""
    r = records_of(F.synthetic_photons(n, seed, n_identifiers=1, **kwargs))
    r["stringID"], r["omID"] = -1, 25
    return r


def tied_records(n, seed):
    """n records equal in (module, tkey, identifier) with n distinct contents: only h and the words put them in order"""
    r = one_module(n, seed, special=False, quantised=False)
    r["time"], r["id"] = 1234.5, 1003
    assert len(np.unique(F.words_of(r), axis=0)) == n
    return r


def colliding_records():
    """two records equal in (module, tkey, identifier, h) with distinct contents: F.colliding_pair()"""
    r = np.zeros(2, dtype=CV.FRAME_PHOTON_DTYPE)
    r["stringID"], r["omID"], r["id"], r["time"] = 1, 25, 1003, 1234.5
    for k, name in enumerate(F.FLOATS):
        r[name] = np.array([w[k] for w in F.colliding_pair()], dtype=np.uint32).view(np.float32)
    assert F.mix(F.words_of(r))[0] == F.mix(F.words_of(r))[1] and r[0].tobytes() != r[1].tobytes()
    return r


def special_time_records(seed=2):
    """records on one module whose times are the special values and the NaNs of NAN_TIME_BITS, under three identifiers"""
    bits = np.concatenate([np.ascontiguousarray(F.SPECIAL_TIMES.astype(np.float64)).view(np.uint64), NAN_TIME_BITS])
    r = one_module(6 * len(bits), seed, special=False)
    r["time"] = np.tile(bits, 6).view(np.float64)
    r["id"] = 1000 + np.arange(len(r)) % 3
    return r


def malformed_cases(doms):
    """name -> (records, series): each breaks one rule of the series form (some cannot help breaking a second one)"""
    records, series = frame_photons_of(doms, bunch(20000, 5))
    assert len(series) > 50 and (series["count"][:16] > 3).all()
    cases = {}
    owner = np.repeat(np.arange(len(series)), series["count"])
    inner = owner[1:] == owner[:-1]
    t, w = F.tkey_of(records["time"]), F.words_of(records)
    h = F.mix(w)

    def case(name, edit):
        r, s = records.copy(), series.copy()
        out = edit(r, s)
        cases[name] = out if out is not None else (r, s)

    def not_ascending(r, s):                    # entry 4 repeats entry 3's (frame, module); its records carry that module, so only the order breaks
        assert s["frame"][3] == s["frame"][4]
        s["stringID"][4], s["omID"][4] = s["stringID"][3], s["omID"][3]
        at = slice(int(s["first"][4]), int(s["first"][4] + s["count"][4]))
        r["stringID"][at], r["omID"][at] = s["stringID"][3], s["omID"][3]
    case("table_not_strictly_ascending", not_ascending)

    def frames_descend(r, s):
        k = int(np.flatnonzero(np.diff(s["frame"].astype(np.int64)) > 0)[0])
        s["frame"][k], s["frame"][k + 1] = s["frame"][k + 1], s["frame"][k]
    case("frames_descend", frames_descend)

    def zero_count(r, s):
        s["count"][7] = 0
    case("count_is_zero", zero_count)

    def first_not_zero(r, s):
        s["first"][0] = 1
        s["count"][0] -= 1
    case("first_entry_does_not_start_at_zero", first_not_zero)

    def gap(r, s):
        s["first"][9] += 1
        s["count"][9] -= 1
    case("entries_do_not_follow_each_other", gap)

    case("last_entry_does_not_end_at_the_records", lambda r, s: (r[:-1].copy(), s))
    case("empty_table_with_records", lambda r, s: (r[:5].copy(), s[:0].copy()))

    def wrong_module(r, s):
        r["omID"][int(s["first"][11]) + 1] += 1
    case("record_of_another_module", wrong_module)

    def swap(i):
        def edit(r, s):
            r[[i, i + 1]] = r[[i + 1, i]]
        return edit

    rising = np.flatnonzero(inner & (t[1:] > t[:-1]))
    case("time_descends", swap(int(rising[len(rising) // 2])))

    def identifier_descends(r, s):
        i = int(s["first"][13])
        r["time"][i + 1] = r["time"][i]
        r["id"][i], r["id"][i + 1] = 1030, 1002
    case("identifier_descends_at_equal_times", identifier_descends)

    # neighbours equal in (tkey, identifier) that differ in h: exchanged, only h descends
    only_h = np.flatnonzero(inner & (t[1:] == t[:-1]) & (records["id"][1:] == records["id"][:-1]) & (h[1:] > h[:-1]))
    assert len(only_h) > 10
    case("h_descends", swap(int(only_h[len(only_h) // 2])))

    def w7_descends(r, s):                      # the first two records of a series become W7_PAIR in descending order, at the series' smallest
        k = next(k for k in range(15, len(s)) if s["count"][k] > 3 and t[s["first"][k] + 2] > t[s["first"][k]])         # (tkey, identifier)
        i = int(s["first"][k])
        for j, w7 in ((i, W7_PAIR[1]), (i + 1, W7_PAIR[0])):
            for name, word in zip(F.FLOATS, W7_PREFIX + (w7,)):
                r[name][j] = np.array([word], dtype=np.uint32).view(np.float32)[0]
            r["time"][j], r["id"][j] = r["time"][i], r["id"][i]
    case("w7_descends", w7_descends)
    return cases


# two payloads that differ in w7 alone and have the same h (found by a birthday search over 2^21 values of w7 behind this prefix)
W7_PREFIX = (0x3f800000, 0x34000000, 0x3e600000, 0x42c80000, 0xc2c80000, 0x41200000, 0x3fc00000)
W7_PAIR = (0x3f5df9dd, 0x4051b28d)
assert F.mix(np.array(W7_PREFIX + W7_PAIR[:1], dtype=np.uint32))[0] == F.mix(np.array(W7_PREFIX + W7_PAIR[1:], dtype=np.uint32))[0]
