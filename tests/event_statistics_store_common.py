"""Shared by tests/test_event_statistics_store.py and tests/test_event_statistics_store_gpu.py: an independent statement of CANON,
COMBINE and SPLIT of the event statistics frame store (include/clsimhip.h, "Event statistics frame store") -- a Python dict keyed by
(frame, identifier) with Python integers: sums modulo 2^384, counts modulo 2^64, special counters modulo 2^32; it shares no code with
clsim_amd/csrc -- and the case generators both test files use."""
import numpy as np

from clsim_amd import converter as CV

TILE = 2048                                     # records per workgroup of the tiled kernels (event_stats_store.h: kEventStatsStoreTile)
LONG_RUN = 16                                   # a run this long is summed by a whole wave (kEventStatsLongRun)
ALL = 0xFFFFFFFF
DTYPE = CV.EVENT_STATISTICS_DTYPE
MAP = CV.RELABEL_DTYPE
M384, M64, M32 = 1 << 384, 1 << 64, 1 << 32
NO_MAP = np.zeros(0, dtype=MAP)


def words_to_int(words):
    return sum(int(w) << (64 * k) for k, w in enumerate(words))


def int_to_words(value):
    return [(value >> (64 * k)) & (M64 - 1) for k in range(6)]


def value_of(rec):
    """the 136 bytes behind the key as Python integers"""
    return (int(rec["generatedCount"]), int(rec["atDOMsCount"]), words_to_int(rec["generatedSum"]), words_to_int(rec["atDOMsSum"]),
            tuple(int(v) for v in rec["generatedSpecial"]), tuple(int(v) for v in rec["atDOMsSpecial"]))


ZERO = (0, 0, 0, 0, (0, 0, 0), (0, 0, 0))


def add(a, b):
    return ((a[0] + b[0]) % M64, (a[1] + b[1]) % M64, (a[2] + b[2]) % M384, (a[3] + b[3]) % M384,
            tuple((x + y) % M32 for x, y in zip(a[4], b[4])), tuple((x + y) % M32 for x, y in zip(a[5], b[5])))


def records_of(table):
    """the statistics form of a dict {(frame, identifier): value}"""
    out = np.zeros(len(table), dtype=DTYPE)
    for k, key in enumerate(sorted(table)):
        v = table[key]
        out[k]["frame"], out[k]["id"] = key
        out[k]["generatedCount"], out[k]["atDOMsCount"] = v[0], v[1]
        out[k]["generatedSum"], out[k]["atDOMsSum"] = int_to_words(v[2]), int_to_words(v[3])
        out[k]["generatedSpecial"], out[k]["atDOMsSpecial"] = v[4], v[5]
    return out


def canon(records, map=NO_MAP):
    """(statistics form, {"relabelled", "empty_dropped"}) of any list of records"""
    to = {int(m["from"]): int(m["to"]) for m in map}
    table, relabelled, empty = {}, 0, 0
    for rec in records:
        v = value_of(rec)
        if v == ZERO:
            empty += 1
            continue
        identifier = int(rec["id"])
        if identifier in to:
            identifier, relabelled = to[identifier], relabelled + 1
        key = (int(rec["frame"]), identifier)
        table[key] = add(table[key], v) if key in table else v
    return records_of(table), {"relabelled": relabelled, "empty_dropped": empty}


def is_form(records):
    keys = [(int(r["frame"]), int(r["id"])) for r in records]
    return all(a < b for a, b in zip(keys, keys[1:])) and all(value_of(r) != ZERO for r in records)


def combine(a, b):
    assert is_form(a) and is_form(b)
    table = {(int(r["frame"]), int(r["id"])): value_of(r) for r in a}
    for r in b:
        key = (int(r["frame"]), int(r["id"]))
        table[key] = add(table[key], value_of(r)) if key in table else value_of(r)
    return records_of(table)


def split(records, last_frame):
    assert is_form(records)
    head = records["frame"].astype(np.int64) <= last_frame
    h = int(head.sum())
    assert head[:h].all()
    return records[:h], records[h:]


def same(got, want):
    assert got.dtype == want.dtype == DTYPE and len(got) == len(want)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


# ---- case generators ----
def random_records(n, seed, identifiers=(1000, 1400), frames=(3, 9, 4, 7, 5), wide=True):
    """n records with identifiers and frames drawn from the given sets, in no order, with duplicates; sums are signed 384-bit values of
    every size (wide) or fit 64 bits"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=DTYPE)
    out["id"] = rng.integers(identifiers[0], identifiers[1], n)
    out["frame"] = np.asarray(frames, dtype=np.uint32)[rng.integers(0, len(frames), n)]
    out["generatedCount"] = rng.integers(0, 1 << 40, n)
    out["atDOMsCount"] = rng.integers(1, 1 << 20, n)
    for name in ("generatedSum", "atDOMsSum"):
        w = rng.integers(0, 1 << 63, (n, 6), dtype=np.uint64) * 2 + rng.integers(0, 2, (n, 6), dtype=np.uint64)
        if wide:
            top = rng.integers(0, 6, n)                 # the highest word in use; half of the values negative (sign-extended)
            negative = rng.integers(0, 2, n).astype(bool)
            for k in range(6):
                w[:, k] = np.where(k > top, np.where(negative, np.uint64(M64 - 1), np.uint64(0)), w[:, k])
        else:
            w[:, 1:] = 0
        out[name] = w
    special = rng.integers(0, 50, n) == 0
    out["generatedSpecial"][special] = rng.integers(0, 4, (int(special.sum()), 3))
    out["atDOMsSpecial"][special] = rng.integers(0, 1 << 32, (int(special.sum()), 3), dtype=np.uint64)
    return out


def distinct_records(n, seed, frames=(3, 9, 4, 7, 5)):
    """n records with n distinct keys, shuffled"""
    out = random_records(n, seed)
    per = max((n + len(frames) - 1) // len(frames), 1)
    out["frame"] = np.asarray(frames, dtype=np.uint32)[np.arange(n) // per]
    out["id"] = 5000 + np.arange(n) % per
    np.random.default_rng(seed + 1).shuffle(out)
    return out


def one_key_records(n, seed, frame=6, identifier=77):
    out = random_records(n, seed)
    out["frame"], out["id"] = frame, identifier
    return out


def runs_records(lengths, seed, frame=2):
    """one run per entry of `lengths`, identifiers 100, 101, ..., the members of all runs shuffled together"""
    out = random_records(int(sum(lengths)), seed)
    out["frame"] = frame
    out["id"] = np.repeat(100 + np.arange(len(lengths)), lengths)
    np.random.default_rng(seed + 1).shuffle(out)
    return out


def empties(n, seed):
    """n empty records with keys of their own"""
    out = np.zeros(n, dtype=DTYPE)
    rng = np.random.default_rng(seed)
    out["id"], out["frame"] = rng.integers(0, 1 << 32, n), rng.integers(0, 10, n)
    return out


def record(frame, identifier, generated=0, at_doms=0, generated_count=0, at_doms_count=1, generated_special=(0, 0, 0), at_doms_special=(0, 0, 0)):
    """one record from Python integers; the sums are taken modulo 2^384 (negative values in two's complement)"""
    out = np.zeros(1, dtype=DTYPE)
    out["frame"], out["id"] = frame, identifier
    out["generatedCount"], out["atDOMsCount"] = generated_count % M64, at_doms_count % M64
    out["generatedSum"], out["atDOMsSum"] = int_to_words(generated % M384), int_to_words(at_doms % M384)
    out["generatedSpecial"], out["atDOMsSpecial"] = generated_special, at_doms_special
    return out


def relabel_map(pairs):
    out = np.zeros(len(pairs), dtype=MAP)
    for k, (a, b) in enumerate(sorted(pairs)):
        out[k]["from"], out[k]["to"] = a, b
    return out


def malformed_cases():
    """name -> (records, index of the first offending element): each breaks one rule of the statistics form"""
    good = canon(random_records(3000, 17))[0]
    assert len(good) > 1500
    cases = {}
    r = good.copy()
    r[[700, 701]] = r[[701, 700]]
    cases["keys_descend"] = (r, 701)
    r = good.copy()
    r[900] = r[899]
    cases["key_repeated"] = (r, 900)
    r = good.copy()
    key = r[1200][["id", "frame"]].copy()
    r[1200] = np.zeros(1, dtype=DTYPE)[0]
    r[1200]["id"], r[1200]["frame"] = key["id"], key["frame"]
    cases["empty_record"] = (r, 1200)
    r = good.copy()
    frames = np.flatnonzero(np.diff(r["frame"].astype(np.int64)) > 0)
    k = int(frames[1]) + 1
    r["frame"][k] = r["frame"][0]
    cases["frame_descends"] = (r, k)
    return cases


MALFORMED = ("keys_descend", "key_repeated", "empty_record", "frame_descends")
