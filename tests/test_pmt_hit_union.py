"""PMT hit frame store on the host: the twins of the union and the split (clsimhip_pmt_hits_union_host / _split_host) against an
independent numpy restatement, the bridge to the PMT series stage -- Union(Series(A), Series(B)) = Series(A ++ B) byte for byte --,
the order of arrival, the split's properties, the host store, the times' bit patterns, the pmt word as an integer, every rule of
the series form of PMT hits refused, and the twins and the host store as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import pmt_photon_hits_common as PH
from tests import pmt_series_common as PS
from tests import pmt_hit_union_common as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
STORE = CV.PMTHitFrameStore
UNION = STORE.UnionHost
SPLIT = STORE.SplitHost
BOUNDS = (0, 9, 10, 15, 20, 29, 30, 40, 49, 50, 51, U.ALL)
REFUSED = CV.I3CLSimStepToPhotonConverter_exception


@pytest.fixture(scope="module")
def gen():
    return PS.synthetic_generator()[0]


@pytest.fixture(scope="module")
def bad(gen):
    cases = U.malformed_cases(gen)
    assert sorted(cases) == sorted(U.MALFORMED)
    return cases


def test_the_header_words_the_definition_once():
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert header.index("---- Frame photon store") < header.index("---- PMT hit frame store") < header.index("---- Cable shadow")
    assert len(re.findall(r"SERIES FORM OF PMT HITS:", header)) == 1
    section = header[header.index("---- PMT hit frame store"):header.index("---- Cable shadow")]
    assert "SERIES FORM:" not in section and "SERIES FORM OF FRAME PHOTONS:" not in section


@pytest.mark.parametrize("n_a,n_b", U.SIZES)
def test_twin_equals_numpy_and_the_series_of_the_whole(gen, n_a, n_b):
    a, b, whole = U.pair(gen, n_a, n_b)
    if n_a + n_b >= 8000:
        assert len(set(whole[1]["frame"])) == 5 and len(whole[0]) < n_a + n_b            # five frames, and the mask took some
        assert (~np.isfinite(whole[0]["time"])).sum() >= 16
    got = UNION(*a, *b)
    U.same(got, U.numpy_union(*a, *b))
    U.same(got, whole)                                                                   # the bridge
    U.same(UNION(*b, *a), whole)
    U.check_form(*got)


def test_seven_parts_in_three_orders_of_arrival(gen):
    h = U.bunch(9000, 8)
    parts = [U.series_of(gen, h[k::7]) for k in range(7)]
    whole = U.series_of(gen, h)
    for order in ((0, 1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1, 0), (3, 0, 6, 1, 5, 2, 4)):
        acc = (whole[0][:0], whole[1][:0])
        for k in order:
            acc = UNION(*acc, *parts[k])
        U.same(acc, whole)
    # ... and as a tree
    U.same(UNION(*UNION(*UNION(*parts[0], *parts[1]), *UNION(*parts[2], *parts[3])), *UNION(*UNION(*parts[4], *parts[5]), *parts[6])), whole)


def test_union_with_itself_doubles_every_count(gen):
    records, series = U.series_of(gen, U.bunch(5000, 2))
    got = UNION(records, series, records, series)
    assert got[0].tobytes() == np.repeat(records, 2).tobytes()
    assert np.array_equal(got[1]["count"], 2 * series["count"]) and np.array_equal(got[1]["first"], 2 * series["first"])
    assert np.array_equal(got[1][["frame", "stringID", "omID", "pmt", "reserved"]], series[["frame", "stringID", "omID", "pmt", "reserved"]])


def test_split_properties(gen):
    records, series = U.series_of(gen, U.bunch(7000, 3))
    sizes = set()
    for bound in BOUNDS:
        head, head_series, tail, tail_series = got = SPLIT(records, series, bound)
        U.same(got, U.numpy_split(records, series, bound))
        U.same(UNION(head, head_series, tail, tail_series), (records, series))
        assert (head_series["frame"].astype(np.int64) <= bound).all() and (tail_series["frame"].astype(np.int64) > bound).all()
        U.check_form(head, head_series)
        U.check_form(tail, tail_series)
        sizes.add(len(head))
    assert len(sizes) == 6 and 0 in sizes and len(records) in sizes
    # a head or a tail that does not fit
    n_head = len(SPLIT(records, series, 30)[0])
    for kwargs in (dict(head_capacity=n_head - 1), dict(tail_capacity=len(records) - n_head - 1)):
        with pytest.raises(REFUSED, match="records, its output") as e:
            SPLIT(records, series, 30, **kwargs)
        assert e.value.code == _lib.ERR_ARGUMENT
    assert len(SPLIT(records, series, 30, head_capacity=n_head, tail_capacity=len(records) - n_head)[0]) == n_head


def test_store_fed_in_parts_equals_the_series_of_all_hits_restricted_to_the_frames(gen):
    h = U.bunch(8000, 6)
    p = U.particles()
    frame_of = dict(zip(p["id"].tolist(), p["frame"].tolist()))
    frames = np.array([frame_of[i] for i in h["id"].tolist()])
    store = STORE(20000)
    assert store.Size() == (0, 0) and len(store.Drain()[0]) == 0
    for k in range(5):
        store.Add(*U.series_of(gen, h[k::5]))
    whole = U.series_of(gen, h)
    assert store.Size() == (len(whole[0]), len(whole[1]))
    for lo, hi in ((0, 20), (20, 20), (20, 40), (40, U.ALL)):
        want = U.series_of(gen, h[(frames > lo) & (frames <= hi)] if lo else h[frames <= hi])
        assert store.Size(hi) == (len(want[0]), len(want[1]))
        U.same(store.Drain(hi), want)
    assert store.Size() == (0, 0)
    # frames that are drained while later parts still arrive: what arrives behind a drain is delivered by the next one
    store = STORE(20000)
    early, late = h[frames <= 20], h[frames > 20]
    fed = np.concatenate([early, late[:1000]])
    for k in range(3):
        store.Add(*U.series_of(gen, fed[k::3]))
    U.same(store.Drain(20), U.series_of(gen, early))
    store.Add(*U.series_of(gen, late[1000:]))
    U.same(store.Drain(), U.series_of(gen, late))


# negative NaNs (signalling, quiet, with payloads), -inf, -0, +0, +inf, positive NaNs (signalling, quiet): ascending in tkey
ORDERED_BITS = np.array([0xFFFFFFFFFFFFFFFF, 0xFFF8000000000001, 0xFFF8000000000000, 0xFFF4000000000000, 0xFFF0000000000001, 0xFFF0000000000000,
                         0xBFF0000000000000, 0x8000000000000000, 0x0000000000000000, 0x3FF0000000000000, 0x7FF0000000000000, 0x7FF0000000000001,
                         0x7FF4000000000000, 0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)


def test_nan_times_of_both_signs_quiet_and_signalling_keep_their_bits():
    n = len(ORDERED_BITS)
    h = np.zeros(2 * n, dtype=CV.PMT_HIT_DTYPE)
    h["id"], h["stringID"], h["omID"], h["pmt"] = 1000, 1, 25, 63
    rng = np.random.default_rng(4)
    h["time"] = np.concatenate([ORDERED_BITS[rng.permutation(n)], ORDERED_BITS[rng.permutation(n)]]).view(np.float64)
    frames = np.full(2 * n, 7, dtype=np.uint32)
    a, b = U.form_of(h[:n], frames[:n]), U.form_of(h[n:], frames[n:])
    assert np.array_equal(a[0]["time"].view(np.uint64), ORDERED_BITS)                    # (the helper's own order: negative NaNs first, positive NaNs last)
    records, series = UNION(*a, *b)
    assert np.array_equal(records["time"].view(np.uint64), np.repeat(ORDERED_BITS, 2))
    assert len(series) == 1 and series["count"][0] == 2 * n
    U.same((records, series), U.numpy_union(*a, *b))
    head, head_series, tail, tail_series = SPLIT(records, series, 7)
    assert np.array_equal(head["time"].view(np.uint64), np.repeat(ORDERED_BITS, 2)) and len(tail) == 0
    store = STORE(100)
    store.Add(*b)
    store.Add(*a)
    U.same(store.Drain(), (records, series))


def test_two_pmt_values_that_differ_only_above_bit_6_are_ordered_as_integers():
    h = np.zeros(6, dtype=CV.PMT_HIT_DTYPE)
    h["id"], h["stringID"], h["omID"] = 1000, -1, 10
    h["pmt"] = (5, 5 + 64, 5 + 128, 5 + (1 << 31), 5 + (1 << 16), 5 + 64)
    h["time"] = (6.0, 5.0, 4.0, 3.0, 2.0, 1.0)
    frames = np.zeros(6, dtype=np.uint32)
    a, b = U.form_of(h[::2], frames[::2]), U.form_of(h[1::2], frames[1::2])
    records, series = UNION(*a, *b)
    assert records["pmt"].tolist() == [5, 69, 69, 133, 5 + (1 << 16), 5 + (1 << 31)]
    assert series["pmt"].tolist() == [5, 69, 133, 5 + (1 << 16), 5 + (1 << 31)] and series["count"].tolist() == [1, 2, 1, 1, 1]
    assert records["time"].tolist() == [6.0, 1.0, 5.0, 4.0, 2.0, 3.0]
    U.same((records, series), U.numpy_union(*a, *b))


@pytest.mark.parametrize("name", U.MALFORMED)
def test_each_malformed_rule_is_refused(gen, bad, name):
    case = bad[name]
    good = U.series_of(gen, U.bunch(500, 1))
    element = "record" if name in U.RECORD_CASES else "entry"
    for call, who in ((lambda: UNION(*case, *good), "A"), (lambda: UNION(*good, *case), "B"), (lambda: SPLIT(*case, 30), "the input of the split")):
        with pytest.raises(REFUSED, match=r"%s is no series form: %s \d+ of" % (who, element)) as e:
            call()
        assert e.value.code == _lib.ERR_ARGUMENT
    store = STORE(30000)
    store.Add(*good)
    with pytest.raises(REFUSED, match="the bunch is no series form") as e:
        store.Add(*case)
    assert e.value.code == _lib.ERR_ARGUMENT
    U.same(store.Drain(), good)


def test_the_first_offending_element_is_named(gen, bad):
    good = U.series_of(gen, U.bunch(500, 1))
    records, series = U.series_of(gen, U.bunch(20000, 5))                               # what the cases were made of
    busy = np.flatnonzero(series["count"] > 3)
    same_module = np.flatnonzero((series["frame"][1:] == series["frame"][:-1]) & (series["stringID"][1:] == series["stringID"][:-1]) &
                                 (series["omID"][1:] == series["omID"][:-1]))
    k_pmt = int(same_module[4]) + 1
    ascending = bad["table_not_strictly_ascending"][1]
    assert (ascending["frame"][k_pmt - 1], ascending["stringID"][k_pmt - 1], ascending["omID"][k_pmt - 1]) == \
           (ascending["frame"][k_pmt], ascending["stringID"][k_pmt], ascending["omID"][k_pmt]) and ascending["pmt"][k_pmt - 1] > ascending["pmt"][k_pmt]
    for name, text in (("count_is_zero", "entry 7 of"), ("first_entry_does_not_start_at_zero", "entry 0 of"), ("entries_do_not_follow_each_other", "entry 9 of"),
                       ("table_not_strictly_ascending", "entry %d of" % k_pmt), ("entry_reserved_nonzero", "entry 11 of"), ("empty_table_with_records", "record 0 of 5"),
                       ("last_entry_does_not_end_at_the_records", "entry %d of" % (len(series) - 1)),
                       ("record_of_another_dom", "record %d of" % (int(series["first"][busy[3]]) + 1)),
                       ("record_of_another_pmt", "record %d of" % (int(series["first"][busy[4]]) + 1)),
                       ("record_reserved_nonzero", "record %d of" % (int(series["first"][busy[5]]) + 2)),
                       ("identifier_descends_at_equal_times", "record %d of" % (int(series["first"][busy[6]]) + 1))):
        with pytest.raises(REFUSED, match=text):
            UNION(*bad[name], *good)
        with pytest.raises(REFUSED, match="B is no series form: " + text):
            UNION(*good, *bad[name])
    # an output that does not fit
    with pytest.raises(REFUSED, match="the union holds %d records, the output %d" % (2 * len(good[0]), 2 * len(good[0]) - 1)) as e:
        UNION(*good, *good, capacity=2 * len(good[0]) - 1)
    assert e.value.code == _lib.ERR_ARGUMENT


def drain_status(store, last_frame, capacity):
    records, series = np.zeros(capacity, dtype=CV.PMT_HIT_DTYPE), np.zeros(capacity, dtype=CV.PMT_SERIES_DTYPE)
    n, n_series = C.c_size_t(), C.c_size_t()
    return _lib.load().clsimhip_pmt_hit_store_drain_host(store._h, last_frame, records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity,
                                                         C.byref(n), C.byref(n_series))


def test_a_host_store_at_capacity_refuses_the_bunch_that_does_not_fit_and_keeps_its_content(gen):
    first = U.series_of(gen, U.bunch(3000, 1))
    second = U.series_of(gen, U.bunch(1500, 2))
    store = STORE(len(first[0]) + len(second[0]) - 1)
    store.Add(*first)
    with pytest.raises(REFUSED, match="does not fit") as e:
        store.Add(*second)
    assert e.value.code == _lib.ERR_ARGUMENT
    assert store.Size() == (len(first[0]), len(first[1]))
    store.Add(second[0][:0], second[1][:0])                                              # an empty bunch fits anywhere
    head = SPLIT(*second, 20)[:2]
    store.Add(*head)
    U.same(store.Drain(), UNION(*first, *head))
    # device calls on a host store, a capacity beyond 2^31
    for call in (lambda: store.AddDevice(16, 16, 16, 1), lambda: store.DrainDevice(0, 16, 16, 16, 1)):
        with pytest.raises(REFUSED) as e:
            call()
        assert e.value.code == _lib.ERR_STATE
    with pytest.raises(REFUSED, match="2\\^31") as e:
        STORE(2 ** 31 + 1)
    assert e.value.code == _lib.ERR_ARGUMENT
    # a drain into too small an output leaves the store as it was
    store.Add(*first)
    assert drain_status(store, U.ALL, len(first[0]) - 1) == _lib.ERR_ARGUMENT and store.Size() == (len(first[0]), len(first[1]))


def test_the_photon_hits_stage_output_is_a_bunch_and_unions_with_a_series_stage_output():
    """clsimhip_pmt_photon_hits_host's output (hits made of stored frame photons, whose times pass through bit for bit: signalling
    NaNs among them) with clsimhip_pmt_series_host's, for the same modules and frames"""
    gen = PS.synthetic_generator()[0]
    from_photons = gen.MakeHitsFromFramePhotonsHost(*PH.synthetic_records(4000, 17))[:2]
    assert len(from_photons[0]) > 100
    bits = set(from_photons[0]["time"].view(np.uint64).tolist())
    assert 0x7FF0000000000001 in bits or 0xFFF4000000000002 in bits                     # a signalling NaN made it into a hit
    records, series, _ = gen.MakeSeriesHost(U.bunch(3000, 12), PS.particle_table(U.IDENTIFIERS))       # the frames of PH.synthetic_records
    from_series = (records, series)
    assert set(from_photons[1]["frame"].tolist()) == set(from_series[1]["frame"].tolist())
    got = UNION(*from_photons, *from_series)
    U.same(got, U.numpy_union(*from_photons, *from_series))
    U.same(UNION(*from_series, *from_photons), got)
    U.check_form(*got)
    store = STORE(len(got[0]))
    store.Add(*from_series)
    store.Add(*from_photons)
    U.same(store.Drain(), got)


# ---- the stand-alone host program under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/pmt_hit_union_host_main.cpp and clsim_amd/csrc/pmt_hit_union.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("pmt_hit_union_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c", os.path.join(ROOT, "clsim_amd", "csrc", "pmt_hit_union.cpp"),
                                                                         os.path.join(ROOT, "tests", "pmt_hit_union_host_main.cpp")], cwd=str(d))
    exe = str(d / "pmt_hit_union_host_main")
    # (linked without the HIP runtime: the twins and the host store make no HIP call)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "pmt_hit_union.o", "pmt_hit_union_host_main.o", "-o", exe],
                          cwd=str(d))
    return exe


def form(records, series):
    return struct.pack("<2Q", len(records), len(series)) + np.ascontiguousarray(records).tobytes() + np.ascontiguousarray(series).tobytes()


class Reader:
    def __init__(self, blob):
        self.blob, self.at = blob, 0

    def u64(self):
        v = struct.unpack_from("<Q", self.blob, self.at)[0]
        self.at += 8
        return v

    def form(self):
        n, n_series = self.u64(), self.u64()
        records = np.frombuffer(self.blob, dtype=CV.PMT_HIT_DTYPE, count=n, offset=self.at)
        self.at += 24 * n
        series = np.frombuffer(self.blob, dtype=CV.PMT_SERIES_DTYPE, count=n_series, offset=self.at)
        self.at += 24 * n_series
        return records, series


def test_host_program_runs_clean_under_the_sanitizers(gen, bad, host_program, tmp_path):
    a, b, whole = U.pair(gen, 2049, 6145)
    empty = (whole[0][:0], whole[1][:0])
    q = lambda *v: struct.pack("<%dQ" % len(v), *v)
    commands = [q(1, len(whole[0])) + form(*a) + form(*b),                              # exactly the capacity it needs
                q(1, 0) + form(*empty) + form(*empty),
                q(1, len(whole[0]) - 1) + form(*a) + form(*b),                          # one short of it: refused
                q(2, 30, len(whole[0]), len(whole[0])) + form(*whole),
                q(2, U.ALL, len(whole[0]), 0) + form(*whole),
                q(2, 0, 0, len(whole[0])) + form(*whole),
                q(3, len(whole[0])), q(4) + form(*a), q(6, 30), q(5, 20, len(a[0])), q(4) + form(*b), q(4) + form(*b),     # the second one does not fit
                q(5, U.ALL, 1),                                                         # refused: too small an output
                q(5, U.ALL, len(whole[0]))]
    commands += [q(1, 30000) + form(*bad[name]) + form(*a) for name in sorted(bad)]
    commands += [q(2, 30, 30000, 30000) + form(*bad[name]) for name in sorted(bad)]
    commands += [q(4) + form(*bad[name]) for name in sorted(bad)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(commands))
    run = subprocess.run([host_program, src, dst], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    assert run.stdout.strip() == "%d commands, %d refused" % (len(commands), 3 + 3 * len(bad))
    r = Reader(open(dst, "rb").read())
    refused = -_lib.ERR_ARGUMENT                                                        # the status word
    assert r.u64() == 0
    U.same(r.form(), whole)
    assert r.u64() == 0
    U.same(r.form(), empty)
    assert r.u64() == refused
    for bound in (30, U.ALL, 0):
        assert r.u64() == 0
        want = U.numpy_split(*whole, bound)
        U.same(r.form() + r.form(), want)
    assert r.u64() == 0 and r.u64() == 0                                                # store, add
    head_a = U.numpy_split(*a, 30)
    assert (r.u64(), r.u64(), r.u64()) == (0, len(head_a[0]), len(head_a[1]))           # size
    assert r.u64() == 0
    head_20 = U.numpy_split(*a, 20)
    U.same(r.form(), head_20[:2])
    assert r.u64() == 0 and r.u64() == refused and r.u64() == refused
    assert r.u64() == 0
    U.same(r.form(), UNION(*head_20[2:], *b))
    assert [r.u64() for _ in range(3 * len(bad))] == [refused] * (3 * len(bad))
    assert r.at == len(r.blob)
