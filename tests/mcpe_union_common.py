"""Shared by tests/test_mcpe_union.py and tests/test_mcpe_union_gpu.py: an independent numpy restatement of the union and the split
of the MCPE frame store (include/clsimhip.h, "MCPE frame store"), the synthetic inputs both test files use, and one crafted input
per rule of the series form."""
import numpy as np

from clsim_amd import converter as CV
from tests import mcpe_series_common as S

FRAMES = (50, 10, 40, 20, 30)
MASK = S.mask_of([(10, 1, 10), (50, -3, 60), (30, 86, 30)])
SIZES = [(0, 0), (0, 100), (100, 0), (63, 65), (2049, 6145), (20000, 300)]
ALL = 0xFFFFFFFF


def frames_of(series):
    return np.repeat(series["frame"], series["count"])


def table_of(records, frame):
    """the series table of records that ascend in (frame, DOM code, ...)"""
    code = S.dom_code(records["stringID"], records["omID"])
    head = np.ones(len(records), dtype=bool)
    head[1:] = (frame[1:] != frame[:-1]) | (code[1:] != code[:-1])
    first = np.flatnonzero(head)
    series = np.zeros(len(first), dtype=CV.MCPE_SERIES_DTYPE)
    series["frame"], series["stringID"], series["omID"], series["first"] = frame[first], records["stringID"][first], records["omID"][first], first
    series["count"] = np.diff(np.append(first, len(records)))
    return series


def numpy_union(a_records, a_series, b_records, b_series):
    """np.lexsort on (identifier, tkey, DOM code, frame) of the concatenation; the table from the heads"""
    records = np.concatenate([a_records, b_records])
    frame = np.concatenate([frames_of(a_series), frames_of(b_series)])
    order = np.lexsort((records["id"], S.tkey_of(records["time"]), S.dom_code(records["stringID"], records["omID"]), frame))
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


def bunch(n, seed, **kwargs):
    """n synthetic MCPEs with the special times, and the particle table that deals their identifiers to five frames"""
    m = S.synthetic_mcpes(n, seed, **kwargs)
    return m, S.particle_table(np.arange(1000, 1040), frames=FRAMES)


def series_of(gen, mcpes):
    records, series, _ = gen.MakeSeriesHost(mcpes, S.particle_table(np.arange(1000, 1040), frames=FRAMES), MASK)
    return records, series


def pair(gen, n_a, n_b, seed=21):
    """the series of the two parts of one bunch of n_a + n_b MCPEs (the mask takes a few away), and of the whole"""
    m, _ = bunch(n_a + n_b, seed)
    return series_of(gen, m[:n_a]), series_of(gen, m[n_a:]), series_of(gen, m)


def one_dom(n, seed):
    """n MCPEs on one DOM in one frame: one series"""
    m = S.synthetic_mcpes(n, seed, n_identifiers=1)
    m["stringID"], m["omID"] = -1, 25
    return m


def malformed_cases(gen):
    """name -> (records, series): each breaks one rule of the series form (some cannot help breaking a second one)"""
    records, series = series_of(gen, bunch(20000, 5)[0])
    assert len(series) > 50 and (series["count"][:16] > 3).all()
    cases = {}

    def case(name, edit):
        r, s = records.copy(), series.copy()
        out = edit(r, s)
        cases[name] = out if out is not None else (r, s)

    def not_ascending(r, s):                    # entry 4 repeats entry 3's (frame, DOM); its records carry that DOM, so only the order breaks
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

    def wrong_dom(r, s):
        r["omID"][int(s["first"][11]) + 1] += 1
    case("record_of_another_dom", wrong_dom)

    def time_descends(r, s):
        t = S.tkey_of(r["time"])
        inside = np.flatnonzero((np.repeat(np.arange(len(s)), s["count"])[1:] == np.repeat(np.arange(len(s)), s["count"])[:-1]) & (t[1:] > t[:-1]))
        i = int(inside[len(inside) // 2])
        r["time"][i], r["time"][i + 1] = r["time"][i + 1], r["time"][i]
        r["id"][i], r["id"][i + 1] = r["id"][i + 1], r["id"][i]
    case("time_descends", time_descends)

    def identifier_descends(r, s):
        i = int(s["first"][13])
        r["time"][i + 1] = r["time"][i]
        r["id"][i], r["id"][i + 1] = 1030, 1002
        assert S.tkey_of(r["time"][i + 1:i + 3])[0] <= S.tkey_of(r["time"][i + 1:i + 3])[1]
    case("identifier_descends_at_equal_times", identifier_descends)
    return cases


def form_of(mcpes, frames):
    """the series form of records with the frame of each given: np.lexsort, no table, no mask, no shift -- every record is kept"""
    mcpes, frames = np.ascontiguousarray(mcpes, dtype=CV.MCPE_DTYPE), np.asarray(frames, dtype=np.uint32)
    order = np.lexsort((mcpes["id"], S.tkey_of(mcpes["time"]), S.dom_code(mcpes["stringID"], mcpes["omID"]), frames))
    return mcpes[order], table_of(mcpes[order], frames[order])


def exact_pair(n_a, n_b, seed=31):
    """two series forms of exactly n_a and n_b records over the same frames and DOMs"""
    m = S.synthetic_mcpes(n_a + n_b, seed)
    frames = np.asarray(FRAMES, dtype=np.uint32)[m["id"] % len(FRAMES)]
    return form_of(m[:n_a], frames[:n_a]), form_of(m[n_a:], frames[n_a:])
