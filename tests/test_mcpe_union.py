"""MCPE frame store on the host: the twins of the union and the split (clsimhip_mcpe_series_union_host / _split_host) against an
independent numpy restatement, the bridge to the series stage -- Union(Series(A), Series(B)) = Series(A ++ B) byte for byte --, the
order of arrival, the split's properties, the host store, every rule of the series form refused, and the twins and the host store
as a stand-alone program under the sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import mcpe_series_common as S
from tests import mcpe_union_common as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
UNION = CV.MCPEGenerator.UnionHost
SPLIT = CV.MCPEGenerator.SplitHost
MERGE = CV.MCPEGenerator.MergeHost
BOUNDS = (0, 9, 10, 15, 20, 29, 30, 40, 49, 50, 51, U.ALL)


@pytest.fixture(scope="module")
def gen():
    return S.synthetic_generator()


def test_the_header_words_the_definition_once():
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert header.index("---- MCPE merging") < header.index("---- MCPE frame store") < header.index("---- Multi-PMT hit generator")
    assert len(re.findall(r"SERIES FORM:", header)) == 1 and "lastPendingFrame" in header


@pytest.mark.parametrize("n_a,n_b", U.SIZES)
def test_twin_equals_numpy_and_the_series_of_the_whole(gen, n_a, n_b):
    a, b, whole = U.pair(gen, n_a, n_b)
    if n_a + n_b >= 8000:
        assert len(set(whole[1]["frame"])) == 5 and len(whole[0]) < n_a + n_b            # five frames, and the mask took some
    if n_a + n_b >= 8000:
        assert (~np.isfinite(whole[0]["time"])).sum() >= 16
    got = UNION(*a, *b)
    U.same(got, U.numpy_union(*a, *b))
    U.same(got, whole)                                                                   # the bridge
    U.same(UNION(*b, *a), whole)
    if len(got[1]):                                                                      # (the helper takes no empty table)
        S.check_properties(*got)


def test_seven_parts_in_three_orders_of_arrival(gen):
    m, _ = U.bunch(9000, 8)
    parts = [U.series_of(gen, m[k::7]) for k in range(7)]
    whole = U.series_of(gen, m)
    for order in ((0, 1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1, 0), (3, 0, 6, 1, 5, 2, 4)):
        acc = (whole[0][:0], whole[1][:0])
        for k in order:
            acc = UNION(*acc, *parts[k])
        U.same(acc, whole)
    # ... and as a tree
    U.same(UNION(*UNION(*UNION(*parts[0], *parts[1]), *UNION(*parts[2], *parts[3])), *UNION(*UNION(*parts[4], *parts[5]), *parts[6])), whole)


def test_union_with_itself_doubles_every_count(gen):
    records, series = U.series_of(gen, U.bunch(5000, 2)[0])
    got = UNION(records, series, records, series)
    assert got[0].tobytes() == np.repeat(records, 2).tobytes()
    assert np.array_equal(got[1]["count"], 2 * series["count"]) and np.array_equal(got[1]["first"], 2 * series["first"])
    assert np.array_equal(got[1][["frame", "stringID", "omID"]], series[["frame", "stringID", "omID"]])


def test_split_properties(gen):
    records, series = U.series_of(gen, U.bunch(7000, 3)[0])
    sizes = set()
    for bound in BOUNDS:
        head, head_series, tail, tail_series = got = SPLIT(records, series, bound)
        U.same(got, U.numpy_split(records, series, bound))
        U.same(UNION(head, head_series, tail, tail_series), (records, series))
        assert (head_series["frame"].astype(np.int64) <= bound).all() and (tail_series["frame"].astype(np.int64) > bound).all()
        for part in ((head, head_series), (tail, tail_series)):
            if len(part[1]):
                S.check_properties(*part)
        sizes.add(len(head))
    assert len(sizes) == 6 and 0 in sizes and len(records) in sizes
    # a head or a tail that does not fit
    n_head = len(SPLIT(records, series, 30)[0])
    for kwargs in (dict(head_capacity=n_head - 1), dict(tail_capacity=len(records) - n_head - 1)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="records, its output") as e:
            SPLIT(records, series, 30, **kwargs)
        assert e.value.code == _lib.ERR_ARGUMENT
    assert len(SPLIT(records, series, 30, head_capacity=n_head, tail_capacity=len(records) - n_head)[0]) == n_head


def fed_in_parts(store, gen, m, parts, drains):
    """feeds the bunch in `parts` parts; drains[k]: the bound drained behind part k.  Returns what was drained, in order"""
    out = []
    for k in range(parts):
        store.Add(*U.series_of(gen, m[k::parts]))
        if k in drains:
            out.append(store.Drain(drains[k]))
    return out


def test_store_fed_in_parts_equals_the_series_of_all_mcpes_restricted_to_the_frames(gen):
    m, p = U.bunch(8000, 6)
    frame_of = dict(zip(p["id"].tolist(), p["frame"].tolist()))
    frames = np.array([frame_of[i] for i in m["id"].tolist()])
    store = CV.MCPEFrameStore(20000)
    assert store.Size() == (0, 0) and len(store.Drain()[0]) == 0
    for k in range(5):
        store.Add(*U.series_of(gen, m[k::5]))
    whole = U.series_of(gen, m)
    assert store.Size() == (len(whole[0]), len(whole[1]))
    for lo, hi in ((0, 20), (20, 20), (20, 40), (40, U.ALL)):
        want = U.series_of(gen, m[(frames > lo) & (frames <= hi)] if lo else m[frames <= hi])
        assert store.Size(hi) == (len(want[0]), len(want[1]))
        window = 25.0
        U.same(store.DrainMerged(hi, window), MERGE(*want, window))
    assert store.Size() == (0, 0)
    # frames that are drained while later parts still arrive: what arrives behind a drain is delivered by the next one
    store = CV.MCPEFrameStore(20000)
    early = m[frames <= 20]
    late = m[frames > 20]
    got = fed_in_parts(store, gen, np.concatenate([early, late[:1000]]), 3, {2: 20})
    U.same(got[0], U.series_of(gen, early))
    store.Add(*U.series_of(gen, late[1000:]))
    U.same(store.Drain(), U.series_of(gen, late))


@pytest.mark.parametrize("name", ["table_not_strictly_ascending", "frames_descend", "count_is_zero", "first_entry_does_not_start_at_zero",
                                  "entries_do_not_follow_each_other", "last_entry_does_not_end_at_the_records", "empty_table_with_records",
                                  "record_of_another_dom", "time_descends", "identifier_descends_at_equal_times"])
def test_each_malformed_rule_is_refused(gen, name):
    cases = U.malformed_cases(gen)
    assert sorted(cases) == sorted(test_each_malformed_rule_is_refused.pytestmark[0].args[1])
    bad = cases[name]
    good = U.series_of(gen, U.bunch(500, 1)[0])
    element = "record" if name in ("empty_table_with_records", "record_of_another_dom", "time_descends", "identifier_descends_at_equal_times") else "entry"
    for call, who in ((lambda: UNION(*bad, *good), "A"), (lambda: UNION(*good, *bad), "B"), (lambda: SPLIT(*bad, 30), "the input of the split")):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=r"%s is no series form: %s \d+ of" % (who, element)) as e:
            call()
        assert e.value.code == _lib.ERR_ARGUMENT
    store = CV.MCPEFrameStore(10000)
    store.Add(*good)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="the bunch is no series form") as e:
        store.Add(*bad)
    assert e.value.code == _lib.ERR_ARGUMENT
    U.same(store.Drain(), good)


def test_the_first_offending_element_is_named(gen):
    cases = U.malformed_cases(gen)
    good = U.series_of(gen, U.bunch(500, 1)[0])
    for name, text in (("count_is_zero", "entry 7 of"), ("first_entry_does_not_start_at_zero", "entry 0 of"), ("entries_do_not_follow_each_other", "entry 9 of"),
                       ("table_not_strictly_ascending", "entry 4 of"), ("empty_table_with_records", "record 0 of 5")):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=text):
            UNION(*cases[name], *good)
    records, series = cases["record_of_another_dom"]
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="record %d of" % (int(series["first"][11]) + 1)):
        UNION(*good, records, series)
    # an output that does not fit
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="the union holds %d records, the output %d" % (2 * len(good[0]), 2 * len(good[0]) - 1)) as e:
        UNION(*good, *good, capacity=2 * len(good[0]) - 1)
    assert e.value.code == _lib.ERR_ARGUMENT


def test_a_host_store_at_capacity_refuses_the_bunch_that_does_not_fit_and_keeps_its_content(gen):
    first = U.series_of(gen, U.bunch(3000, 1)[0])
    second = U.series_of(gen, U.bunch(1500, 2)[0])
    store = CV.MCPEFrameStore(len(first[0]) + len(second[0]) - 1)
    store.Add(*first)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="does not fit") as e:
        store.Add(*second)
    assert e.value.code == _lib.ERR_ARGUMENT
    assert store.Size() == (len(first[0]), len(first[1]))
    store.Add(second[0][:0], second[1][:0])                                              # an empty bunch fits anywhere
    head = SPLIT(*second, 20)[:2]
    store.Add(*head)
    U.same(store.Drain(), UNION(*first, *head))
    # device calls on a host store, a capacity beyond 2^31
    for call in (lambda: store.AddDevice(16, 16, 16, 1), lambda: store.DrainDevice(0, 16, 16, 16, 1)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            call()
        assert e.value.code == _lib.ERR_STATE
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="2\\^31") as e:
        CV.MCPEFrameStore(2 ** 31 + 1)
    assert e.value.code == _lib.ERR_ARGUMENT
    # a drain into too small an output leaves the store as it was
    store.Add(*first)
    h = C_drain(store, U.ALL, len(first[0]) - 1)
    assert h == _lib.ERR_ARGUMENT and store.Size() == (len(first[0]), len(first[1]))


def C_drain(store, last_frame, capacity):
    import ctypes as C
    records, series = np.zeros(capacity, dtype=CV.MCPE_DTYPE), np.zeros(capacity, dtype=CV.MCPE_SERIES_DTYPE)
    n, n_series = C.c_size_t(), C.c_size_t()
    return _lib.load().clsimhip_mcpe_frame_store_drain_host(store._h, last_frame, records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity,
                                                            C.byref(n), C.byref(n_series))


# ---- the stand-alone host program under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/mcpe_union_host_main.cpp and clsim_amd/csrc/mcpe_union.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("mcpe_union_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c", os.path.join(ROOT, "clsim_amd", "csrc", "mcpe_union.cpp"),
                                                                         os.path.join(ROOT, "tests", "mcpe_union_host_main.cpp")], cwd=str(d))
    exe = str(d / "mcpe_union_host_main")
    # (linked without the HIP runtime: the twins and the host store make no HIP call)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "mcpe_union.o", "mcpe_union_host_main.o", "-o", exe], cwd=str(d))
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
        records = np.frombuffer(self.blob, dtype=CV.MCPE_DTYPE, count=n, offset=self.at)
        self.at += 16 * n
        series = np.frombuffer(self.blob, dtype=CV.MCPE_SERIES_DTYPE, count=n_series, offset=self.at)
        self.at += 16 * n_series
        return records, series


def test_host_program_runs_clean_under_the_sanitizers(gen, host_program, tmp_path):
    a, b, whole = U.pair(gen, 2049, 6145)
    empty = (whole[0][:0], whole[1][:0])
    bad = U.malformed_cases(gen)
    q = lambda *v: struct.pack("<%dQ" % len(v), *v)
    commands = [q(1, len(whole[0])) + form(*a) + form(*b),                              # exactly the capacity it needs
                q(1, 0) + form(*empty) + form(*empty),
                q(1, len(whole[0]) - 1) + form(*a) + form(*b),                          # refused: does not fit
                q(2, 30, len(whole[0]), len(whole[0])) + form(*whole),
                q(2, U.ALL, len(whole[0]), 0) + form(*whole),
                q(2, 0, 0, len(whole[0])) + form(*whole),
                q(3, len(whole[0])), q(4) + form(*a), q(6, 30), q(5, 20, len(a[0])), q(4) + form(*b), q(4) + form(*b),     # the second one does not fit
                q(5, U.ALL, 1),                                                         # refused: too small an output
                q(5, U.ALL, len(whole[0]))]
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
    assert [r.u64() for _ in range(3 * len(bad))] == [-_lib.ERR_ARGUMENT] * (3 * len(bad))
    assert r.at == len(r.blob)
