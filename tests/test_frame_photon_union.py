"""Frame photon store on the host: the twins of the union and the split (clsimhip_frame_photons_union_host / _split_host) against an
independent numpy restatement, the bridge to the frame photons stage -- Union(FramePhotons(A), FramePhotons(B)) = FramePhotons(A ++ B)
byte for byte --, a run of content ties beyond the stage's bound, the order of arrival, the split's properties, the host store in
front of the photon hits twin, every rule of the series form refused, and the twins and the host store as a stand-alone program
under the sanitizers.  Every comparison is byte equality."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import frame_photon_union_common as U
from tests import frame_photons_common as F
from tests import photon_hits_common as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
UNION = CV.FramePhotonStore.UnionHost
SPLIT = CV.FramePhotonStore.SplitHost
BOUNDS = (0, 9, 10, 15, 20, 29, 30, 40, 49, 50, 51, U.ALL)
MALFORMED = ["table_not_strictly_ascending", "frames_descend", "count_is_zero", "first_entry_does_not_start_at_zero", "entries_do_not_follow_each_other",
             "last_entry_does_not_end_at_the_records", "empty_table_with_records", "record_of_another_module", "time_descends",
             "identifier_descends_at_equal_times", "h_descends", "w7_descends"]
RECORD_RULES = ("empty_table_with_records", "record_of_another_module", "time_descends", "identifier_descends_at_equal_times", "h_descends", "w7_descends")
Refused = CV.I3CLSimStepToPhotonConverter_exception


@pytest.fixture(scope="module")
def doms():
    return F.synthetic_doms()


@pytest.fixture(scope="module")
def malformed(doms):
    return U.malformed_cases(doms)


def test_the_header_words_the_definition_behind_frame_photons():
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert header.index("---- Frame photons") < header.index("---- Frame photon store") < header.index("---- Cable shadow")
    assert "NO TIE BOUND" in header and len(re.findall(r"SERIES FORM OF FRAME PHOTONS:", header)) == 1


@pytest.mark.parametrize("n_a,n_b", U.SIZES)
def test_twin_equals_numpy_and_the_frame_photons_of_the_whole(doms, n_a, n_b):
    a, b, whole = U.pair(doms, n_a, n_b)
    if n_a + n_b >= 8000:
        assert len(set(whole[1]["frame"])) == 5 and len(whole[0]) < n_a + n_b           # five frames, and the mask took some
        assert (~np.isfinite(whole[0]["time"])).sum() >= 16 and F.content_ties(whole[0]) > 50
    got = UNION(*a, *b)
    U.same(got, U.numpy_union(*a, *b))
    U.same(got, whole)                                                                   # the bridge
    U.same(UNION(*b, *a), whole)
    F.check_properties(*got)


def test_nan_times_of_both_signs_quiet_and_signalling_keep_their_bits():
    r = U.special_time_records()
    frames = np.full(len(r), 6, dtype=np.uint32)
    a, b = U.form_of(r[0::2], frames[0::2]), U.form_of(r[1::2], frames[1::2])
    got = UNION(*a, *b)
    U.same(got, U.numpy_union(*a, *b))
    U.same(got, U.form_of(r, frames))
    bits = got[0]["time"].view(np.uint64)
    assert set(U.NAN_TIME_BITS.tolist()) <= set(bits.tolist())                          # every payload is still there, signalling ones too
    assert bits[0] == 0xFFFFFFFFFFFFFFFF and bits[-1] == 0x7FFFFFFFFFFFFFFF             # negative NaNs first, positive NaNs last
    head, head_series, tail, tail_series = SPLIT(*got, 6)
    U.same((head, head_series), got)
    assert len(tail) == 0 and len(tail_series) == 0


def test_no_tie_bound(doms):
    """a run of 3 000 records equal in (frame, module, tkey, identifier, h) with two contents: the stage on the whole reports
    TIE_OVERFLOW; each half of 1 500 is within the stage's bound, and the union of the halves' outputs is the full order"""
    m = F.collision_run(3000, 4)
    at = np.flatnonzero((m["stringID"] == 1) & (m["omID"] == 25) & (m["id"] == 1003) & (m["t"] == np.float32(1234.5)))
    assert len(at) >= 3000
    in_a = np.ones(len(m), dtype=bool)
    in_a[at[1500:]] = False
    p = F.particle_table(m["id"])
    whole = doms.MakeFramePhotonsHost(m, p)
    assert whole[2]["tie_overflow"] >= 3000 and len(whole[0]) == 0
    a, b = doms.MakeFramePhotonsHost(m[in_a], p), doms.MakeFramePhotonsHost(m[~in_a], p)
    assert a[2]["tie_overflow"] == b[2]["tie_overflow"] == 0 and len(a[0]) + len(b[0]) == len(m)
    got = UNION(*a[:2], *b[:2])
    U.same(got, U.numpy_union(*a[:2], *b[:2]))
    F.check_properties(*got)
    h = F.mix(F.words_of(got[0]))
    run = np.flatnonzero((got[0]["stringID"] == 1) & (got[0]["omID"] == 25) & (got[0]["id"] == 1003) & (h == F.mix(F.colliding_pair()[0])[0]))
    w = F.words_of(got[0][run])
    assert len(run) == 3000 and (np.diff(run) == 1).all() and len(np.unique(got[0]["time"][run])) == 1 and len(np.unique(w, axis=0)) == 2
    changes = int((w[1:] != w[:-1]).any(axis=1).sum())
    assert changes == 1                                                                  # one content, then the other: ordered by the words


def test_seven_parts_in_three_orders_of_arrival(doms):
    m = U.bunch(9000, 8)
    parts = [U.frame_photons_of(doms, m[k::7]) for k in range(7)]
    whole = U.frame_photons_of(doms, m)
    for order in ((0, 1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1, 0), (3, 0, 6, 1, 5, 2, 4)):
        acc = (whole[0][:0], whole[1][:0])
        for k in order:
            acc = UNION(*acc, *parts[k])
        U.same(acc, whole)
    # ... and as a tree
    U.same(UNION(*UNION(*UNION(*parts[0], *parts[1]), *UNION(*parts[2], *parts[3])), *UNION(*UNION(*parts[4], *parts[5]), *parts[6])), whole)


def test_union_with_itself_doubles_every_count(doms):
    records, series = U.frame_photons_of(doms, U.bunch(5000, 2))
    got = UNION(records, series, records, series)
    assert got[0].tobytes() == np.repeat(records, 2).tobytes()
    assert np.array_equal(got[1]["count"], 2 * series["count"]) and np.array_equal(got[1]["first"], 2 * series["first"])
    assert np.array_equal(got[1][["frame", "stringID", "omID"]], series[["frame", "stringID", "omID"]])


def test_split_properties(doms):
    records, series = U.frame_photons_of(doms, U.bunch(7000, 3))
    sizes = set()
    for bound in BOUNDS:
        head, head_series, tail, tail_series = got = SPLIT(records, series, bound)
        U.same(got, U.numpy_split(records, series, bound))
        U.same(UNION(head, head_series, tail, tail_series), (records, series))
        assert (head_series["frame"].astype(np.int64) <= bound).all() and (tail_series["frame"].astype(np.int64) > bound).all()
        F.check_properties(head, head_series)
        F.check_properties(tail, tail_series)
        sizes.add(len(head))
    assert len(sizes) == 6 and 0 in sizes and len(records) in sizes
    # a head or a tail that does not fit
    n_head = len(SPLIT(records, series, 30)[0])
    for kwargs in (dict(head_capacity=n_head - 1), dict(tail_capacity=len(records) - n_head - 1)):
        with pytest.raises(Refused, match="records, its output") as e:
            SPLIT(records, series, 30, **kwargs)
        assert e.value.code == _lib.ERR_ARGUMENT
    assert len(SPLIT(records, series, 30, head_capacity=n_head, tail_capacity=len(records) - n_head)[0]) == n_head


def test_store_fed_in_parts_in_front_of_the_photon_hits_twin(doms):
    m = U.bunch(8000, 6)
    m["weight"] = np.where(np.arange(len(m)) % 11 == 0, 0.0, 1.0)
    p = U.particles()
    frame_of = dict(zip(p["id"].tolist(), p["frame"].tolist()))
    frames = np.array([frame_of[i] for i in m["id"].tolist()])
    maker = P.maker_of(P.keep_all(F.DOM_STRINGS, F.DOM_OMS, pancake=2.0))
    store = CV.FramePhotonStore(20000)
    assert store.Size() == (0, 0) and len(store.Drain()[0]) == 0
    for k in range(5):
        store.Add(*U.frame_photons_of(doms, m[k::5]))
    whole = U.frame_photons_of(doms, m)
    assert store.Size() == (len(whole[0]), len(whole[1]))
    for lo, hi in ((0, 20), (20, 20), (20, 40), (40, U.ALL)):
        want = U.frame_photons_of(doms, m[(frames > lo) & (frames <= hi)] if lo else m[frames <= hi])
        assert store.Size(hi) == (len(want[0]), len(want[1]))
        P.same(store.DrainHits(hi, maker), maker.MakeHitsHost(*want))
    assert store.Size() == (0, 0)
    # the whole at once
    store.Add(*U.frame_photons_of(doms, m[:3000]))
    store.Add(*U.frame_photons_of(doms, m[3000:]))
    hits = store.DrainHits(U.ALL, maker)
    assert len(hits[0]) > 1000
    P.same(hits, maker.MakeHitsHost(*whole))
    # frames that are drained while later parts still arrive: what arrives behind a drain is delivered by the next one
    early, late = m[frames <= 20], m[frames > 20]
    first = np.concatenate([early, late[:1000]])
    for k in range(3):
        store.Add(*U.frame_photons_of(doms, first[k::3]))
    U.same(store.Drain(20), U.frame_photons_of(doms, early))
    store.Add(*U.frame_photons_of(doms, late[1000:]))
    U.same(store.Drain(), U.frame_photons_of(doms, late))


@pytest.mark.parametrize("name", MALFORMED)
def test_each_malformed_rule_is_refused(doms, malformed, name):
    assert sorted(malformed) == sorted(MALFORMED)
    bad = malformed[name]
    good = U.frame_photons_of(doms, U.bunch(500, 1))
    element = "record" if name in RECORD_RULES else "entry"
    for call, who in ((lambda: UNION(*bad, *good), "A"), (lambda: UNION(*good, *bad), "B"), (lambda: SPLIT(*bad, 30), "the input of the split")):
        with pytest.raises(Refused, match=r"%s is no series form: %s \d+ of" % (who, element)) as e:
            call()
        assert e.value.code == _lib.ERR_ARGUMENT
    store = CV.FramePhotonStore(10000)
    store.Add(*good)
    with pytest.raises(Refused, match="the bunch is no series form") as e:
        store.Add(*bad)
    assert e.value.code == _lib.ERR_ARGUMENT
    U.same(store.Drain(), good)


def first_difference(bad, good):
    return int(np.flatnonzero((bad.view(np.uint8).reshape(len(bad), -1) != good.view(np.uint8).reshape(len(good), -1)).any(axis=1))[0])


def test_the_first_offending_element_is_named(doms, malformed):
    good = U.frame_photons_of(doms, U.bunch(500, 1))
    for name, text in (("count_is_zero", "entry 7 of"), ("first_entry_does_not_start_at_zero", "entry 0 of"), ("entries_do_not_follow_each_other", "entry 9 of"),
                       ("table_not_strictly_ascending", "entry 4 of"), ("empty_table_with_records", "record 0 of 5")):
        with pytest.raises(Refused, match=text):
            UNION(*malformed[name], *good)
    records, series = malformed["record_of_another_module"]
    with pytest.raises(Refused, match="record %d of" % (int(series["first"][11]) + 1)):
        UNION(*good, records, series)
    # the rules on the suffix: the second record of the pair that was exchanged (or crafted) is the first that descends
    whole = U.frame_photons_of(doms, U.bunch(20000, 5))[0]
    for name in ("time_descends", "h_descends", "w7_descends"):
        i = first_difference(malformed[name][0], whole)
        with pytest.raises(Refused, match="record %d of" % (i + 1)):
            UNION(*malformed[name], *good)
    # the pair of "w7_descends" is equal in everything in front of w7, h included; that of "h_descends" in (tkey, identifier)
    r = malformed["w7_descends"][0]
    i = first_difference(r, whole)
    w = F.words_of(r[i:i + 2])
    assert r["time"][i] == r["time"][i + 1] and r["id"][i] == r["id"][i + 1] and F.mix(w)[0] == F.mix(w)[1] and (w[0, :7] == w[1, :7]).all() and w[0, 7] > w[1, 7]
    r = malformed["h_descends"][0]
    i = first_difference(r, whole)
    w = F.words_of(r[i:i + 2])
    assert r["time"][i] == r["time"][i + 1] and r["id"][i] == r["id"][i + 1] and F.mix(w)[0] > F.mix(w)[1]
    # an output that does not fit
    with pytest.raises(Refused, match="the union holds %d records, the output %d" % (2 * len(good[0]), 2 * len(good[0]) - 1)) as e:
        UNION(*good, *good, capacity=2 * len(good[0]) - 1)
    assert e.value.code == _lib.ERR_ARGUMENT


def test_a_host_store_at_capacity_refuses_the_bunch_that_does_not_fit_and_keeps_its_content(doms):
    first = U.frame_photons_of(doms, U.bunch(3000, 1))
    second = U.frame_photons_of(doms, U.bunch(1500, 2))
    store = CV.FramePhotonStore(len(first[0]) + len(second[0]) - 1)
    store.Add(*first)
    with pytest.raises(Refused, match="does not fit") as e:
        store.Add(*second)
    assert e.value.code == _lib.ERR_ARGUMENT
    assert store.Size() == (len(first[0]), len(first[1]))
    store.Add(second[0][:0], second[1][:0])                                              # an empty bunch fits anywhere
    head = SPLIT(*second, 20)[:2]
    store.Add(*head)
    U.same(store.Drain(), UNION(*first, *head))
    # device calls on a host store, a capacity beyond 2^31
    for call in (lambda: store.AddDevice(16, 16, 16, 1), lambda: store.DrainDevice(0, 16, 16, 16, 1)):
        with pytest.raises(Refused) as e:
            call()
        assert e.value.code == _lib.ERR_STATE
    with pytest.raises(Refused, match="2\\^31") as e:
        CV.FramePhotonStore(2 ** 31 + 1)
    assert e.value.code == _lib.ERR_ARGUMENT
    # a drain into too small an output leaves the store as it was
    store.Add(*first)
    assert C_drain(store, U.ALL, len(first[0]) - 1) == _lib.ERR_ARGUMENT and store.Size() == (len(first[0]), len(first[1]))


def C_drain(store, last_frame, capacity):
    import ctypes as C
    records, series = np.zeros(capacity, dtype=CV.FRAME_PHOTON_DTYPE), np.zeros(capacity, dtype=CV.MCPE_SERIES_DTYPE)
    n, n_series = C.c_size_t(), C.c_size_t()
    return _lib.load().clsimhip_frame_photon_store_drain_host(store._h, last_frame, records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity,
                                                              C.byref(n), C.byref(n_series))


# ---- the stand-alone host program under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/frame_photon_union_host_main.cpp and clsim_amd/csrc/frame_photon_union.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("frame_photon_union_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c", os.path.join(ROOT, "clsim_amd", "csrc", "frame_photon_union.cpp"),
                                                                         os.path.join(ROOT, "tests", "frame_photon_union_host_main.cpp")], cwd=str(d))
    exe = str(d / "frame_photon_union_host_main")
    # (linked without the HIP runtime: the twins and the host store make no HIP call)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "frame_photon_union.o",
                           "frame_photon_union_host_main.o", "-o", exe], cwd=str(d))
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
        records = np.frombuffer(self.blob, dtype=CV.FRAME_PHOTON_DTYPE, count=n, offset=self.at)
        self.at += 48 * n
        series = np.frombuffer(self.blob, dtype=CV.MCPE_SERIES_DTYPE, count=n_series, offset=self.at)
        self.at += 16 * n_series
        return records, series


def test_host_program_runs_clean_under_the_sanitizers(doms, malformed, host_program, tmp_path):
    a, b, whole = U.pair(doms, 2049, 6145)
    empty = (whole[0][:0], whole[1][:0])
    bad = malformed
    r = U.special_time_records()
    nans = U.form_of(r, np.full(len(r), 6, dtype=np.uint32))
    q = lambda *v: struct.pack("<%dQ" % len(v), *v)
    commands = [q(1, len(whole[0])) + form(*a) + form(*b),                              # exactly the capacity it needs
                q(1, 0) + form(*empty) + form(*empty),
                q(1, len(whole[0]) - 1) + form(*a) + form(*b),                          # refused: does not fit
                q(2, 30, len(whole[0]), len(whole[0])) + form(*whole),
                q(2, U.ALL, len(whole[0]), 0) + form(*whole),
                q(2, 0, 0, len(whole[0])) + form(*whole),
                q(3, len(whole[0])), q(4) + form(*a), q(6, 30), q(5, 20, len(a[0])), q(4) + form(*b), q(4) + form(*b),     # the second one does not fit
                q(5, U.ALL, 1),                                                         # refused: too small an output
                q(5, U.ALL, len(whole[0])),
                q(1, 2 * len(nans[0])) + form(*nans) + form(*nans)]
    commands += [q(1, 20000) + form(*bad[name]) + form(*a) for name in sorted(bad)]
    commands += [q(2, 30, 20000, 20000) + form(*bad[name]) for name in sorted(bad)]
    commands += [q(4) + form(*bad[name]) for name in sorted(bad)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(commands))
    run = subprocess.run([host_program, src, dst], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    assert run.stdout.strip() == "%d commands, %d refused" % (len(commands), 3 + 3 * len(bad))
    r = Reader(open(dst, "rb").read())
    assert r.u64() == 0
    U.same(r.form(), whole)
    assert r.u64() == 0
    U.same(r.form(), empty)
    assert r.u64() == -_lib.ERR_ARGUMENT
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
    assert r.u64() == 0 and r.u64() == -_lib.ERR_ARGUMENT and r.u64() == -_lib.ERR_ARGUMENT
    assert r.u64() == 0
    U.same(r.form(), UNION(*head_20[2:], *b))
    assert r.u64() == 0
    U.same(r.form(), U.numpy_union(*nans, *nans))
    assert [r.u64() for _ in range(3 * len(bad))] == [-_lib.ERR_ARGUMENT] * (3 * len(bad))
    assert r.at == len(r.blob)
