"""Shared by tests/test_series_relabel.py and tests/test_series_relabel_gpu.py: an independent numpy statement of RELABEL
(include/clsimhip.h, "Series relabel") -- the identifiers replaced through np.searchsorted, np.lexsort on the full key, the
disturbed runs found from neighbours -- and the inputs both files use, for the two record types ("mcpe", "photon")."""
import functools

import numpy as np

from clsim_amd import converter as CV
from tests import frame_photon_union_common as FU
from tests import frame_photons_common as F
from tests import mcpe_series_common as S
from tests import mcpe_union_common as U

KINDS = ("mcpe", "photon")
DTYPE = {"mcpe": CV.MCPE_DTYPE, "photon": CV.FRAME_PHOTON_DTYPE}
BOUND = 2048
RUNS = (1, 2, 63, 64, 65, 2048, 2049)


def relabel_map(pairs):
    m = np.zeros(len(pairs), dtype=CV.RELABEL_DTYPE)
    for i, (a, b) in enumerate(pairs):
        m[i] = (a, b)
    return m


def new_ids(ids, m):
    at = np.searchsorted(m["from"], ids)
    hit = (at < len(m)) & (m["from"][np.minimum(at, max(len(m) - 1, 0))] == ids) if len(m) else np.zeros(len(ids), dtype=bool)
    out = ids.copy()
    out[hit] = m["to"][at[hit]]
    return out, int(hit.sum())


def rest_descends(kind, records):
    """per record i >= 1: the rest of the key (identifier; for photons h, w0 ... w7 behind it) of i is below that of i - 1"""
    cols = [records["id"].astype(np.int64)]
    if kind == "photon":
        w = F.words_of(records)
        cols += [F.mix(w).astype(np.int64)] + [w[:, k].astype(np.int64) for k in range(8)]
    less, equal = np.zeros(len(records) - 1, dtype=bool), np.ones(len(records) - 1, dtype=bool)
    for c in cols:
        less |= equal & (c[1:] < c[:-1])
        equal &= c[1:] == c[:-1]
    return less


def disturbed_runs(kind, records, series):
    """(lengths of the disturbed runs, number of runs) of records that already carry their new identifiers, in the input's order"""
    if len(records) == 0:
        return np.zeros(0, dtype=np.int64), 0
    owner = np.repeat(np.arange(len(series)), series["count"])
    t = S.tkey_of(records["time"])
    head = np.ones(len(records), dtype=bool)
    head[1:] = (owner[1:] != owner[:-1]) | (t[1:] != t[:-1])
    run = np.cumsum(head) - 1
    descends = np.zeros(len(records), dtype=bool)
    descends[1:] = ~head[1:] & rest_descends(kind, records)
    lengths = np.bincount(run)
    return lengths[np.unique(run[descends])], int(head.sum())


def numpy_relabel(kind, records, series, m):
    """(records, series, counts): counts as the device writes them -- records, series, RELABELLED, 0, TIE_OVERFLOW"""
    records, series = np.ascontiguousarray(records, dtype=DTYPE[kind]).copy(), np.ascontiguousarray(series, dtype=CV.MCPE_SERIES_DTYPE)
    records["id"], relabelled = new_ids(records["id"], m)
    lengths, _ = disturbed_runs(kind, records, series)
    overflow = int(lengths[lengths > BOUND].sum())
    if overflow:
        return records[:0], series[:0], (0, 0, relabelled, 0, overflow)
    owner = np.repeat(np.arange(len(series)), series["count"])          # (the table is kept: the series, not its frame, is the leading key)
    if kind == "mcpe":
        order = np.lexsort((records["id"], S.tkey_of(records["time"]), owner))
    else:
        w = F.words_of(records)
        order = np.lexsort(tuple(w[:, k] for k in range(7, -1, -1)) + (F.mix(w), records["id"], F.tkey_of(records["time"]), owner))
    return records[order], series.copy(), (len(records), len(series), relabelled, 0, 0)


def host(kind, records, series, m):
    r = CV.SeriesRelabeler(m)
    out, table, counters = (r.mcpe_series_host if kind == "mcpe" else r.frame_photons_host)(records, series)
    return out, table, (len(out), len(table), counters["relabelled"], 0, counters["tie_overflow"])


def same(got, want):
    assert got[2] == tuple(want[2]), (got[2], want[2])
    for g, w in zip(got[:2], want[:2]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


def form_of(kind, records, frames):
    return (U.form_of if kind == "mcpe" else FU.form_of)(records, frames)


@functools.lru_cache(maxsize=None)
def _contents(n):
    return FU.tied_records(n, 7)


def blank(kind, n, string_id=1, om_id=25):
    """n records at one DOM; photons with n distinct contents"""
    r = np.zeros(n, dtype=DTYPE[kind])
    if kind == "photon" and n:
        r[:] = _contents(max(n, 8))[:n]
    r["stringID"], r["omID"] = string_id, om_id
    return r


def run_case(kind, length, disturbed, frame=7):
    """one series: three records in front, `length` records at one time under identifiers 1001 and 1005, three behind.  The map sends
    1005 in front of 1001 (disturbed; a run of one cannot be) or between 1001 and 1006 (undisturbed, yet relabelled)"""
    r = blank(kind, length + 6)
    r["time"] = np.concatenate([[10.0, 11.0, 12.0], np.full(length, 20.0), [30.0, 31.0, 32.0]])
    r["id"] = np.concatenate([[1005, 1001, 1009], np.where(np.arange(length) < length // 2, 1001, 1005), [1001, 1005, 1005]])
    records, series = form_of(kind, r, np.full(len(r), frame, dtype=np.uint32))
    return records, series, relabel_map([(1005, 1000 if disturbed else 1003), (1009, 4)])


def boundary_case(kind):
    """one DOM in two frames, equal times on both sides of the series boundary: the runs must not join"""
    r = blank(kind, 4)
    r["time"], r["id"] = 20.0, [1001, 1005, 1001, 1005]
    records, series = form_of(kind, r, np.array([1, 1, 2, 2], dtype=np.uint32))
    assert len(series) == 2
    return records, series, relabel_map([(1005, 1000)])


def zero_and_nan_case(kind):
    """-0.0 / +0.0 and NaN times: runs are equal bit patterns"""
    r = blank(kind, 8)
    r["time"] = np.array([0x8000000000000000, 0x8000000000000000, 0, 0, 0x7FF8000000000000, 0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000],
                         dtype=np.uint64).view(np.float64)
    r["id"] = [1001, 1005, 1002, 1005, 1001, 1005, 1000, 1005]
    records, series = form_of(kind, r, np.zeros(8, dtype=np.uint32))
    return records, series, relabel_map([(1005, 1000)])


def duplicates_case(kind):
    """two slices of one muon that already has records in the run: equal bytes afterwards (for MCPEs), and a disturbed run"""
    r = blank(kind, 5)
    if kind == "photon":
        r[:] = r[0]                                                     # one content, so that the results are copies
    r["time"], r["id"] = 20.0, [1001, 1003, 1005, 1006, 1006]
    records, series = form_of(kind, r, np.zeros(5, dtype=np.uint32))
    return records, series, relabel_map([(1005, 1001), (1006, 1001)])


def extreme_identifiers_case(kind):
    r = blank(kind, 6)
    r["time"], r["id"] = [1.0, 1.0, 1.0, 2.0, 2.0, 2.0], [0, 5, 0xFFFFFFFF, 0, 5, 0xFFFFFFFF]
    records, series = form_of(kind, r, np.zeros(6, dtype=np.uint32))
    return records, series, relabel_map([(0, 0xFFFFFFFE), (0xFFFFFFFF, 1)])


# ---- random series forms built by the existing host stages ----
MUONS = np.arange(1000, 1010)
SLICES = np.arange(1010, 1040)
SLICE_MAP = relabel_map([(int(s), int(1000 + s % 10)) for s in SLICES])


def particles():
    """the muons and, with their muon's frame and shift, the slices"""
    p = S.particle_table(np.arange(1000, 1040), frames=U.FRAMES)
    p["frame"][10:], p["timeShift"][10:] = p["frame"][SLICES % 10], p["timeShift"][SLICES % 10]
    return p


def random_form(kind, stage, n, seed):
    """(raw, records, series): the series stage's output for n raw records under identifiers 1000 ... 1039"""
    raw = S.synthetic_mcpes(n, seed) if kind == "mcpe" else F.synthetic_photons(n, seed)
    # 240 records at one DOM and four times under all forty identifiers: muons and slices of other muons meet in one run (identifiers
    # equal modulo 5 share frame and shift), so that the map disturbs runs
    k = np.arange(240)
    raw["stringID"][:240], raw["omID"][:240], raw["id"][:240] = 1, 25, 1000 + k % 40
    raw["time" if kind == "mcpe" else "t"][:240] = 1000.0 + (k // 40) % 4
    if kind == "mcpe":
        records, series, counters = stage.MakeSeriesHost(raw, particles(), U.MASK)
    else:
        records, series, counters = stage.MakeFramePhotonsHost(raw, particles(), FU.MASK)
        assert counters["tie_overflow"] == 0
    assert counters["unknown_particle"] == 0
    return raw, records, series


def series_of(kind, stage, raw):
    out = stage.MakeSeriesHost(raw, particles(), U.MASK) if kind == "mcpe" else stage.MakeFramePhotonsHost(raw, particles(), FU.MASK)
    return out[0], out[1]


def has_a_disturbed_run(kind, records, series, m):
    r = records.copy()
    r["id"], _ = new_ids(r["id"], m)
    return len(disturbed_runs(kind, r, series)[0]) > 0


def stage_of(kind):
    return S.synthetic_generator() if kind == "mcpe" else F.synthetic_doms()
