"""Shared by tests/test_pmt_hit_union.py and tests/test_pmt_hit_union_gpu.py: an independent numpy restatement of the union and the
split of the PMT hit frame store (include/clsimhip.h, "PMT hit frame store"), the synthetic inputs both test files use, and one
crafted input per rule of the series form of PMT hits."""
import numpy as np

from clsim_amd import converter as CV
from tests import pmt_series_common as PS

TILE = 2048                                     # records per workgroup of the union's merge (mcpe_series.h: kSeriesTile)
FRAMES = (50, 10, 40, 20, 30)
MASK = PS.mask_of([(10, 1, 10), (50, -3, 60), (30, 86, 30)])
SIZES = [(0, 0), (0, 100), (100, 0), (63, 65), (2049, 6145), (20000, 300)]
# on and beside a tile boundary
GPU_SIZES = [(0, 0), (0, 1), (1, 0), (1, 1), (63, 1), (63, 65), (64, 64), (65, 63), (TILE - 1, 0), (0, TILE), (TILE - 1, 1), (TILE - 1, 2), (1, TILE - 1),
             (TILE, 1), (TILE + 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1), (3 * TILE + 1, TILE - 1), (65, 3 * TILE + 1), (3 * TILE + 1, 3 * TILE + 1)]
ALL = 0xFFFFFFFF
IDENTIFIERS = np.arange(1000, 1040)


def particles():
    return PS.particle_table(IDENTIFIERS, frames=FRAMES)


def frames_of(series):
    return np.repeat(series["frame"], series["count"])


def table_of(records, frame):
    """the series table of records that ascend in (frame, module code, pmt, ...)"""
    code = PS.module_code(records["stringID"], records["omID"])
    head = np.ones(len(records), dtype=bool)
    head[1:] = (frame[1:] != frame[:-1]) | (code[1:] != code[:-1]) | (records["pmt"][1:] != records["pmt"][:-1])
    first = np.flatnonzero(head)
    series = np.zeros(len(first), dtype=CV.PMT_SERIES_DTYPE)
    series["frame"], series["stringID"], series["omID"], series["pmt"] = frame[first], records["stringID"][first], records["omID"][first], records["pmt"][first]
    series["first"] = first
    series["count"] = np.diff(np.append(first, len(records)))
    return series


def order_of(records, frame):
    return np.lexsort((records["id"], PS.tkey_of(records["time"]), records["pmt"], PS.module_code(records["stringID"], records["omID"]), frame))


def numpy_union(a_records, a_series, b_records, b_series):
    """np.lexsort on (identifier, tkey, pmt, module code, frame) of the concatenation; the table from the heads"""
    records = np.concatenate([a_records, b_records])
    frame = np.concatenate([frames_of(a_series), frames_of(b_series)])
    order = order_of(records, frame)
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
        assert g.dtype == w.dtype and np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))


def bunch(n, seed, **kwargs):
    """n synthetic hits with the special times; particles() deals their identifiers to five frames"""
    return PS.synthetic_hits(n, seed, **kwargs)


def series_of(gen, hits):
    records, series, _ = gen.MakeSeriesHost(hits, particles(), MASK)
    return records, series


def pair(gen, n_a, n_b, seed=21):
    """the PMT series of the two parts of one bunch of n_a + n_b hits (the mask takes a few away), and of the whole"""
    h = bunch(n_a + n_b, seed)
    return series_of(gen, h[:n_a]), series_of(gen, h[n_a:]), series_of(gen, h)


def form_of(hits, frames):
    """the series form of records with the frame of each given: np.lexsort, no table, no mask, no shift -- every record is kept,
    every time keeps its bits"""
    hits, frames = np.ascontiguousarray(hits, dtype=CV.PMT_HIT_DTYPE), np.asarray(frames, dtype=np.uint32)
    order = order_of(hits, frames)
    return hits[order], table_of(hits[order], frames[order])


def frames_by_identifier(hits):
    return np.asarray(FRAMES, dtype=np.uint32)[hits["id"] % len(FRAMES)]


def exact_pair(n_a, n_b, seed=31, hits=None):
    """two series forms of exactly n_a and n_b records over the same frames and channels"""
    h = PS.synthetic_hits(n_a + n_b, seed) if hits is None else hits
    frames = frames_by_identifier(h)
    return form_of(h[:n_a], frames[:n_a]), form_of(h[n_a:], frames[n_a:])


def malformed_cases(gen):
    """name -> (records, series): each breaks one rule of the series form of PMT hits (some cannot help breaking a second one)"""
    records, series = series_of(gen, bunch(20000, 5))
    assert len(series) > 200
    busy = np.flatnonzero(series["count"] > 3)              # entries with records to spare
    assert len(busy) > 16
    cases = {}

    def case(name, edit):
        r, s = records.copy(), series.copy()
        out = edit(r, s)
        cases[name] = out if out is not None else (r, s)

    def records_of(s, k):
        return slice(int(s["first"][k]), int(s["first"][k] + s["count"][k]))

    # two neighbours in one (frame, module): they tie in (frame, DOM) and ascend in pmt
    same_module = np.flatnonzero((series["frame"][1:] == series["frame"][:-1]) & (series["stringID"][1:] == series["stringID"][:-1]) &
                                 (series["omID"][1:] == series["omID"][:-1]))
    assert len(same_module) > 8
    k_pmt = int(same_module[4]) + 1

    def not_ascending(r, s):                    # entries k - 1 and k tie in (frame, DOM) and now DESCEND in pmt; the records follow their entries
        s["pmt"][k_pmt - 1], s["pmt"][k_pmt] = s["pmt"][k_pmt], s["pmt"][k_pmt - 1]
        r["pmt"][records_of(s, k_pmt - 1)] = s["pmt"][k_pmt - 1]
        r["pmt"][records_of(s, k_pmt)] = s["pmt"][k_pmt]
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
        s["count"][0] += 1 if s["count"][0] == 1 else -1
    case("first_entry_does_not_start_at_zero", first_not_zero)

    def gap(r, s):
        s["first"][9] += 1
    case("entries_do_not_follow_each_other", gap)

    case("last_entry_does_not_end_at_the_records", lambda r, s: (r[:-1].copy(), s))
    case("empty_table_with_records", lambda r, s: (r[:5].copy(), s[:0].copy()))

    def wrong_dom(r, s):
        r["omID"][int(s["first"][busy[3]]) + 1] += 1
    case("record_of_another_dom", wrong_dom)

    def wrong_pmt(r, s):
        r["pmt"][int(s["first"][busy[4]]) + 1] ^= 64         # differs only above bit 6
    case("record_of_another_pmt", wrong_pmt)

    def record_reserved(r, s):
        r["reserved"][int(s["first"][busy[5]]) + 2] = 1
    case("record_reserved_nonzero", record_reserved)

    def entry_reserved(r, s):
        s["reserved"][11] = 0x80000000
    case("entry_reserved_nonzero", entry_reserved)

    def time_descends(r, s):
        t = PS.tkey_of(r["time"])
        owner = np.repeat(np.arange(len(s)), s["count"])
        inside = np.flatnonzero((owner[1:] == owner[:-1]) & (t[1:] > t[:-1]))
        i = int(inside[len(inside) // 2])
        r["time"][i], r["time"][i + 1] = r["time"][i + 1], r["time"][i]
        r["id"][i], r["id"][i + 1] = r["id"][i + 1], r["id"][i]
    case("time_descends", time_descends)

    def identifier_descends(r, s):
        i = int(s["first"][busy[6]])
        r["time"][i + 1] = r["time"][i]
        r["id"][i], r["id"][i + 1] = 1030, 1002
        assert PS.tkey_of(r["time"][i + 1:i + 3])[0] <= PS.tkey_of(r["time"][i + 1:i + 3])[1]
    case("identifier_descends_at_equal_times", identifier_descends)
    return cases


# where the first offender of a case lies (cases built by malformed_cases)
MALFORMED = ("table_not_strictly_ascending", "frames_descend", "count_is_zero", "first_entry_does_not_start_at_zero", "entries_do_not_follow_each_other",
             "last_entry_does_not_end_at_the_records", "empty_table_with_records", "record_of_another_dom", "record_of_another_pmt", "record_reserved_nonzero",
             "entry_reserved_nonzero", "time_descends", "identifier_descends_at_equal_times")
RECORD_CASES = ("empty_table_with_records", "record_of_another_dom", "record_of_another_pmt", "record_reserved_nonzero", "time_descends",
                "identifier_descends_at_equal_times")


def check_form(records, series):
    if len(series):
        PS.check_properties(records, series)
    else:
        assert len(records) == 0
