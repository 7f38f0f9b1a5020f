"""Event statistics frame store on the host: the twins of CANON, COMBINE and SPLIT (clsimhip_event_statistics_canonical_host /
_combine_host / _split_host) against the independent Python statement of tests/event_statistics_store_common.py, byte for byte; the
three laws of the definition; every refusal, with its message and with nothing written; the host store fed one set of bunches in every
order; and the twins and the host store as a stand-alone program under the sanitizers."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import event_statistics_store_common as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
STORE = CV.EventStatisticsStore
CANON = STORE.CanonicalHost
COMBINE = STORE.CombineHost
SPLIT = STORE.SplitHost
REFUSED = CV.I3CLSimStepToPhotonConverter_exception
T = E.TILE
# slices 1100 ... 1299 belong to muons 1000 ... 1009 (which have records of their own), 1300 ... 1349 to muon 7 (which has none)
MUONS = E.relabel_map([(s, 1000 + s % 10) for s in range(1100, 1300)] + [(s, 7) for s in range(1300, 1350)] + [(2000000, 5)])


def test_the_header_words_the_definition_once():
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert header.count("---- Event statistics frame store") == 1 and header.count("STATISTICS FORM:") == 1
    assert header.index("---- Series relabel") < header.index("---- Event statistics frame store")
    common = open(os.path.join(ROOT, "clsim_amd", "csrc", "event_stats_store.h")).read()
    assert "kEventStatsStoreTile = %du" % T in common and "kEventStatsLongRun = %du" % E.LONG_RUN in common


@pytest.mark.parametrize("n", [0, 1, 2, 63, 300, 3 * T + 5])
def test_canonical_twin_equals_the_python_statement(n):
    for records in (E.random_records(n, seed=n), E.distinct_records(n, seed=n + 1), E.one_key_records(n, seed=n + 2),
                    np.concatenate([E.random_records(n, seed=n + 3), E.empties(n // 2 + 1, seed=4)])):
        for map in (E.NO_MAP, MUONS):
            want, counted = E.canon(records, map)
            got, counters = CANON(records, map)
            E.same(got, want)
            assert counters == counted and E.is_form(got)
    assert len(CANON(E.empties(n, seed=1))[0]) == 0


def test_arithmetic_carries_wraps_cancellation_and_specials():
    ones = (1 << 384) - 1
    got, _ = CANON(np.concatenate([E.record(1, 5, generated=ones, at_doms=ones), E.record(1, 5, generated=1, at_doms=2)]))
    assert len(got) == 1 and not got["generatedSum"].any() and got["atDOMsSum"][0].tolist() == [1, 0, 0, 0, 0, 0]      # the carry ripples through six words and wraps
    got, _ = CANON(np.concatenate([E.record(1, 5, generated=-12345 << 200, at_doms=7 << 300, at_doms_count=3), E.record(1, 5, generated=12345 << 200, at_doms=-7 << 300, at_doms_count=4)]))
    assert len(got) == 1 and not got["generatedSum"].any() and not got["atDOMsSum"].any() and got["atDOMsCount"][0] == 7    # zero sums, and the record stays
    got, _ = CANON(np.concatenate([E.record(1, 5, generated_count=(1 << 64) - 1, at_doms_count=1 << 63), E.record(1, 5, generated_count=3, at_doms_count=1 << 63)]))
    assert got["generatedCount"][0] == 2 and got["atDOMsCount"][0] == 0 and len(got) == 1
    a = E.record(1, 5, at_doms_count=0, generated_special=(1, 2, 3), at_doms_special=(0xFFFFFFFF, 0, 7))
    got, _ = CANON(np.concatenate([a, a]))
    assert got["generatedSpecial"][0].tolist() == [2, 4, 6] and got["atDOMsSpecial"][0].tolist() == [0xFFFFFFFE, 0, 14]
    # two records that cancel in every field are still not empty themselves, and their sum is a record of zeros that stays a record
    got, _ = CANON(np.concatenate([E.record(1, 5, at_doms_count=1), E.record(1, 5, at_doms_count=-1)]))
    assert len(got) == 1 and E.value_of(got[0]) == E.ZERO


def test_maps_fold_slices_into_their_muon_frame_by_frame():
    records = np.concatenate([E.record(f, i, at_doms=i, at_doms_count=1) for f in (4, 2) for i in (1000, 1100, 1110, 1300, 1301, 9)])
    got, counters = CANON(records, MUONS)
    E.same(got, E.canon(records, MUONS)[0])
    assert counters == {"relabelled": 8, "empty_dropped": 0}
    assert got[["frame", "id"]].tolist() == [(2, 7), (2, 9), (2, 1000), (4, 7), (4, 9), (4, 1000)]             # one `to` in two frames stays two records
    assert got["atDOMsCount"].tolist() == [2, 1, 3, 2, 1, 3] and got["atDOMsSum"][:, 0].tolist() == [2601, 9, 3210, 2601, 9, 3210]
    absent = E.relabel_map([(55, 56)])
    got, counters = CANON(records, absent)
    E.same(got, E.canon(records)[0])
    assert counters["relabelled"] == 0


@pytest.mark.parametrize("n_a,n_b", [(0, 0), (0, 100), (100, 0), (63, 65), (T + 1, 3 * T)])
def test_combine_and_split_twins_equal_the_python_statement(n_a, n_b):
    a, b = E.canon(E.random_records(n_a, seed=7))[0], E.canon(E.random_records(n_b, seed=8, identifiers=(1200, 1700)))[0]
    got = COMBINE(a, b)
    E.same(got, E.combine(a, b))
    E.same(COMBINE(b, a), got)                                                          # COMBINE(A, B) == COMBINE(B, A)
    assert len(got) <= len(a) + len(b) and (n_a < 1000 or n_b < 1000 or len(got) < len(a) + len(b))
    for bound in (0, 2, 3, 4, 6, 9, 10, E.ALL):
        head, tail = SPLIT(got, bound)
        want = E.split(got, bound)
        E.same(head, want[0])
        E.same(tail, want[1])
        E.same(COMBINE(head, tail), got)


def test_the_laws():
    l1, l2 = E.random_records(2500, seed=1), np.concatenate([E.random_records(1500, seed=2), E.empties(40, seed=3)])
    both = np.concatenate([l1, l2])
    for map in (E.NO_MAP, MUONS):
        E.same(COMBINE(CANON(l1, map)[0], CANON(l2, map)[0]), CANON(both, map)[0])      # COMBINE(CANON(L1), CANON(L2)) == CANON(L1 ++ L2)
        E.same(CANON(both[::-1], map)[0], CANON(both, map)[0])
    E.same(CANON(CANON(both)[0], MUONS)[0], CANON(both, MUONS)[0])                      # fold at add time == fold at drain time
    form = CANON(both)[0]
    E.same(CANON(form)[0], form)


def refused(call, *words):
    with pytest.raises(REFUSED) as err:
        call()
    assert err.value.code == _lib.ERR_ARGUMENT
    for word in words:
        assert word in str(err.value), str(err.value)


def raw_canonical(records, map, out, capacity):
    n = C.c_size_t(12345)
    counters = np.full(2, 99, dtype=np.uint64)
    rc = _lib.load().clsimhip_event_statistics_canonical_host(records.ctypes.data, len(records), map.ctypes.data if len(map) else None, len(map), out.ctypes.data,
                                                              capacity, C.byref(n), counters.ctypes.data)
    return rc, n.value, counters.tolist()


def test_refusals_name_the_offender_and_write_nothing():
    good = CANON(E.random_records(500, seed=3))[0]
    for name, (records, at) in E.malformed_cases().items():
        text = "record %d of %d" % (at, len(records))
        refused(lambda: COMBINE(records, good), "A is no statistics form", text)
        refused(lambda: COMBINE(good, records), "B is no statistics form", text)
        refused(lambda: SPLIT(records, 5), "the input of the split", text)
        CANON(records)                                                                  # any list is CANON's input
    assert sorted(E.malformed_cases()) == sorted(E.MALFORMED)
    records = E.random_records(300, seed=5)
    refused(lambda: CANON(records, np.array([(5, 1), (5, 2)], dtype=E.MAP)), "not strictly ascending in `from`", "entry 1")
    refused(lambda: CANON(records, np.array([(9, 1), (5, 2)], dtype=E.MAP)), "not strictly ascending in `from`")
    refused(lambda: CANON(records, np.array([(5, 8), (8, 2)], dtype=E.MAP)), "entry 0", "sends 5 to 8")
    # capacity one too small, and nothing written by any refused call
    n = len(CANON(records)[0])
    out = np.full(n, 0xA5, dtype=np.uint8).repeat(144).view(E.DTYPE)
    rc, made, counters = raw_canonical(records, E.NO_MAP, out, n - 1)
    assert rc == _lib.ERR_ARGUMENT and made == 12345 and counters == [99, 99] and (out.view(np.uint8) == 0xA5).all()
    assert b"holds %d records, the output %d" % (n, n - 1) in _lib.load().clsimhip_last_error(None)
    rc, made, counters = raw_canonical(records, np.array([(5, 8), (8, 2)], dtype=E.MAP), out, n)
    assert rc == _lib.ERR_ARGUMENT and made == 12345 and (out.view(np.uint8) == 0xA5).all()
    rc, made, counters = raw_canonical(records, E.NO_MAP, out, n)
    assert rc == 0 and made == n and counters == [0, 0]
    a, b = good[::2].copy(), good[1::2].copy()
    refused(lambda: COMBINE(a, b, capacity=len(good) - 1), "holds %d records, the output %d" % (len(good), len(good) - 1))
    E.same(COMBINE(a, b, capacity=len(good)), good)
    h = len(E.split(good, 5)[0])
    assert 0 < h < len(good)
    refused(lambda: SPLIT(good, 5, head_capacity=h - 1), "the head holds %d records" % h)
    refused(lambda: SPLIT(good, 5, tail_capacity=len(good) - h - 1), "the tail holds %d records" % (len(good) - h))
    assert len(SPLIT(good, 5, head_capacity=h, tail_capacity=len(good) - h)[0]) == h


def test_host_store_gives_identical_drains_in_every_order_of_arrival():
    bunches = [E.random_records(900, seed=s) for s in (11, 12, 13)]
    bunches[1] = np.concatenate([bunches[1], E.empties(30, seed=1)])
    whole = np.concatenate(bunches)
    want = E.canon(whole, MUONS)[0]
    drains = []
    for order in itertools.permutations(range(3)):
        at_add, at_drain = STORE(len(whole)), STORE(len(whole))
        for k in order:
            at_add.Add(bunches[k], MUONS)
            at_drain.Add(bunches[k])
        assert at_add.Size() == len(want) and at_drain.Size() == len(E.canon(whole)[0])
        assert at_add.Size(5) == len(E.split(want, 5)[0])
        head = at_add.Drain(5)
        rest = at_add.Drain()
        E.same(np.concatenate([head, rest]), want)
        E.same(head, E.split(want, 5)[0])
        assert at_add.Size() == 0 and len(at_add.Drain()) == 0
        E.same(np.concatenate([at_drain.Drain(5, MUONS), at_drain.Drain(E.ALL, MUONS)]), want)         # folding when the frames leave
        drains.append(head.tobytes() + rest.tobytes())
    assert len(drains) == 6 and len(set(drains)) == 1


def test_host_store_refusals_leave_it_unchanged():
    bunch = E.random_records(400, seed=21)
    n = len(E.canon(bunch)[0])
    store = STORE(n)
    store.Add(bunch)
    other = E.random_records(50, seed=22, identifiers=(50000, 60000))
    refused(lambda: store.Add(other), "in a store of %d" % n)
    refused(lambda: store.Add(bunch, np.array([(5, 8), (8, 2)], dtype=E.MAP)), "sends 5 to 8")
    store.Add(bunch)                                                                    # the same keys again: it fits
    assert store.Size() == n
    out = np.zeros(n, dtype=E.DTYPE)
    got = C.c_size_t(77)
    rc = _lib.load().clsimhip_event_statistics_store_drain_host(store._h, E.ALL, None, 0, out.ctypes.data, n - 1, C.byref(got))
    assert rc == _lib.ERR_ARGUMENT and got.value == 77 and not out.view(np.uint8).any()
    E.same(store.Drain(), E.canon(np.concatenate([bunch, bunch]))[0])
    with pytest.raises(REFUSED) as err:
        store.AddDevice(0, 0, 0)
    assert err.value.code == _lib.ERR_STATE
    with pytest.raises(REFUSED) as err:
        store.DrainDevice(E.ALL, 0, 0, 0)
    assert err.value.code == _lib.ERR_STATE
    with pytest.raises(REFUSED):
        STORE((1 << 31) + 1)


# ---- the stand-alone host program under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/event_statistics_store_host_main.cpp with clsim_amd/csrc/event_stats_store.cpp and the map's check of series_relabel.cpp,
    host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("event_statistics_store_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    sources = [os.path.join(ROOT, "clsim_amd", "csrc", "event_stats_store.cpp"), os.path.join(ROOT, "clsim_amd", "csrc", "series_relabel.cpp"),
               os.path.join(ROOT, "tests", "event_statistics_store_host_main.cpp")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c"] + sources, cwd=str(d))
    exe = str(d / "event_statistics_store_host_main")
    # (linked without the HIP runtime: the twins and the host store make no HIP call)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "event_stats_store.o", "series_relabel.o",
                           "event_statistics_store_host_main.o", "-o", exe], cwd=str(d))
    return exe


def blob(array):
    return struct.pack("<Q", len(array)) + np.ascontiguousarray(array).tobytes()


class Reader:
    def __init__(self, data):
        self.data, self.at = data, 0

    def u64(self):
        v = struct.unpack_from("<Q", self.data, self.at)[0]
        self.at += 8
        return v

    def records(self):
        n = self.u64()
        out = np.frombuffer(self.data, dtype=E.DTYPE, count=n, offset=self.at)
        self.at += 144 * n
        return out


def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path):
    l1, l2 = np.concatenate([E.random_records(2 * T + 9, seed=1), E.empties(33, seed=2)]), E.one_key_records(T + 1, seed=3)
    a, b = E.canon(l1)[0], E.canon(np.concatenate([l1[::3], l2]))[0]
    want, counted = E.canon(l1, MUONS)
    both = E.combine(a, b)
    bad = E.malformed_cases()
    q = lambda *v: struct.pack("<%dQ" % len(v), *v)
    commands = [q(1, len(want)) + blob(MUONS) + blob(l1),                               # exactly the capacity it needs
                q(1, 0) + blob(E.NO_MAP) + blob(l1[:0]),
                q(1, len(want) - 1) + blob(MUONS) + blob(l1),                           # one short of it: refused
                q(1, len(l1)) + blob(np.array([(5, 8), (8, 2)], dtype=E.MAP)) + blob(l1),          # refused
                q(2, len(both)) + blob(a) + blob(b),
                q(2, len(both) - 1) + blob(a) + blob(b),                                # refused
                q(3, 5, len(both), len(both)) + blob(both), q(3, E.ALL, len(both), 0) + blob(both), q(3, 0, 0, len(both)) + blob(both),
                q(4, len(both)), q(5) + blob(E.NO_MAP) + blob(l1), q(7, 5), q(5) + blob(E.NO_MAP) + blob(np.concatenate([l1[::3], l2])),
                q(5) + blob(E.NO_MAP) + blob(E.random_records(10, seed=4, identifiers=(90000, 99999))),        # does not fit: refused
                q(6, E.ALL, 1) + blob(MUONS),                                           # refused: too small an output
                q(6, 5, len(both)) + blob(MUONS), q(6, E.ALL, len(both)) + blob(MUONS)]
    commands += [q(2, 30000) + blob(bad[name][0]) + blob(a) for name in sorted(bad)]
    commands += [q(3, 5, 30000, 30000) + blob(bad[name][0]) for name in sorted(bad)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(commands))
    run = subprocess.run([host_program, src, dst], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    assert run.stdout.strip() == "%d commands, %d refused" % (len(commands), 5 + 2 * len(bad))
    r = Reader(open(dst, "rb").read())
    no = -_lib.ERR_ARGUMENT                                                             # the status word of a refusal
    assert r.u64() == 0
    E.same(r.records(), want)
    assert (r.u64(), r.u64()) == (counted["relabelled"], counted["empty_dropped"])
    assert r.u64() == 0 and len(r.records()) == 0 and (r.u64(), r.u64()) == (0, 0)
    assert r.u64() == no and r.u64() == no
    assert r.u64() == 0
    E.same(r.records(), both)
    assert r.u64() == no
    for bound in (5, E.ALL, 0):
        assert r.u64() == 0
        head, tail = E.split(both, bound)
        E.same(r.records(), head)
        E.same(r.records(), tail)
    assert r.u64() == 0 and r.u64() == 0                                                # the store, the first bunch
    assert r.u64() == 0 and r.u64() == len(E.split(a, 5)[0])
    assert r.u64() == 0 and r.u64() == no and r.u64() == no
    folded = E.canon(both, MUONS)[0]
    assert r.u64() == 0
    E.same(r.records(), E.canon(E.split(both, 5)[0], MUONS)[0])
    assert r.u64() == 0
    E.same(r.records(), E.canon(E.split(both, 5)[1], MUONS)[0])
    assert len(folded) < len(both)
    for _ in range(2 * len(bad)):
        assert r.u64() == no
    assert r.at == len(r.data)
