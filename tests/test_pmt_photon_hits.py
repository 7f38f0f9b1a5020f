"""PMT photon hits, host side: the host twin (clsimhip_pmt_photon_hits_host) against an independent numpy restatement of the
definition (tests/pmt_photon_hits_common.py), byte for byte, on the committed fixtures as frame photons in the three configurations
of tests/pmt_common.py and on synthetic frame photons with special times; the draw-free bridge to the online path (hit maker, then
PMT series); the subset property of the draw; the counters; the properties of the output; the refusals; the stand-alone host
program under AddressSanitizer and UndefinedBehaviorSanitizer.  Every test asserts that its input contains what it claims to cover.
No GPU here (tests/test_pmt_photon_hits_gpu.py has the kernels)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import frame_photons_common as F
from tests import mcpe_common as M
from tests import pmt_common as PC
from tests import pmt_photon_hits_common as Q
from tests import pmt_series_common as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CASES = [(name, cfg) for name in PC.FIXTURES for cfg in PC.CONFIGURATIONS]


def hits_on_two_pmts_in_two_series(hits, series):
    """the condition every fixture x configuration case meets: more than 0 hits, on at least 2 PMT numbers, in at least 2 input series"""
    modules = set(zip(series["frame"].tolist(), series["stringID"].tolist(), series["omID"].tolist()))
    return len(hits) > 0 and len(set(hits["pmt"].tolist())) >= 2 and len(modules) >= 2


@pytest.mark.parametrize("name,cfg", CASES)
def test_twin_equals_numpy_on_the_fixtures(name, cfg):
    """input A: the committed records through clsimhip_frame_photons_host with a particle table, time shifts and a mask"""
    records, series = Q.fixture_records(name)
    layout = PC.configuration(cfg, PC.sphere_radius_of(name))
    gen = PC.make_generator(*layout)
    got = gen.MakeHitsFromFramePhotonsHost(records, series)
    print(name, cfg, len(records), "records", len(got[0]), "hits", len(got[1]), "series", got[2])
    Q.same(got, Q.numpy_hits(records, series, *layout))
    Q.check_properties(got[0], got[1], series)
    assert hits_on_two_pmts_in_two_series(got[0], got[1])
    assert not any(got[2].values())
    # the input: shifted times (no time is a widened binary32 any more), the mask took records away
    assert (records["time"] != records["time"].astype(np.float32).astype(np.float64)).any()
    assert len(records) < len(M.fixture_photons(name))
    # the hits carry the records' times bit for bit
    assert set(got[0]["time"].view(np.uint64).tolist()) <= set(records["time"].view(np.uint64).tolist())


@pytest.mark.parametrize("layout_name", ["keep_all", "synthetic"])
def test_twin_equals_numpy_on_synthetic_records_with_special_times(layout_name):
    """input B: +-0, +-inf and NaN times of both signs, quiet and signalling, come through bit for bit and in the total order"""
    layout = Q.keep_all_layout() if layout_name == "keep_all" else Q.synthetic_layout()
    gen = PC.make_generator(*layout)
    if layout_name == "keep_all":
        records, series, _ = Q.aimed_records(6000, 5, special_times=True)
    else:
        records, series = Q.synthetic_records(6000, 3)
    assert set(Q.SPECIAL_TIME_BITS) <= set(records["time"].view(np.uint64).tolist())
    got = gen.MakeHitsFromFramePhotonsHost(records, series)
    Q.same(got, Q.numpy_hits(records, series, *layout))
    Q.check_properties(got[0], got[1], series)
    assert len(got[0]) > 100 and (got[0]["pmt"] > 31).any()
    if layout_name == "keep_all":
        assert len(got[0]) == len(records) and set(Q.SPECIAL_TIME_BITS) <= set(got[0]["time"].view(np.uint64).tolist())


@pytest.mark.parametrize("name,cfg", CASES)
def test_draw_free_bridge_to_the_online_path(name, cfg):
    """with every weight a NaN both paths accept exactly the photons that meet a PMT from the front: hit maker -> PMT series equals
    frame photons -> this stage, as arrays"""
    photons = M.fixture_photons(name).copy()
    photons["weight"] = np.nan
    p, masked = Q.fixture_bunch(name)
    layout = PC.configuration(cfg, PC.sphere_radius_of(name))
    gen = PC.make_generator(*layout)
    online_hits, online_counters = gen.ConvertHost(photons)
    online = gen.MakeSeriesHost(online_hits, p, masked)
    strings, oms = M.all_pairs()
    records, series, counters = CV.FramePhotonDoms(strings, oms).MakeFramePhotonsHost(photons, p, masked)
    offline = gen.MakeHitsFromFramePhotonsHost(records, series)
    print(name, cfg, len(online[0]), "hits online,", len(offline[0]), "from frame photons")
    assert len(offline[0]) > 0 and counters["masked"] > 0 and online[2]["masked"] > 0
    assert not any(online_counters.values()) and not any(offline[2].values())
    assert online[0].dtype == offline[0].dtype and online[0].tobytes() == offline[0].tobytes()
    assert len(online[1]) == len(offline[1])
    for field in CV.PMT_SERIES_DTYPE.names:
        assert np.array_equal(online[1][field], offline[1][field]), field
    # the order both paths give: frame, module in OMKey order, PMT, tkey, identifier
    PS.check_properties(offline[0], offline[1])
    # the shift was added once, in binary64: every hit's time is a photon's widened time plus its particle's shift
    shift = dict(zip(p["id"].tolist(), p["timeShift"].tolist()))
    sums = {(np.float64(np.float32(t)) + shift[i]) for t, i in zip(photons["t"].tolist(), photons["id"].tolist())}
    assert set(offline[0]["time"].tolist()) <= sums


@pytest.mark.parametrize("name", ["mie", "flasher_led405"])
def test_hits_at_half_the_collection_efficiency_are_a_subset(name):
    records, series = Q.fixture_records(name)
    functions, types, pmts, modules = PC.configuration("two_types", PC.sphere_radius_of(name))
    halved = pmts.copy()
    halved["collectionEfficiency"] = pmts["collectionEfficiency"] * 0.5         # exact
    a = PC.make_generator(functions, types, pmts, modules).MakeHitsFromFramePhotonsHost(records, series)
    b = PC.make_generator(functions, types, halved, modules).MakeHitsFromFramePhotonsHost(records, series)

    def as_set(hits, table):
        owner = np.repeat(np.arange(len(table)), table["count"])
        s = list(zip(table["frame"][owner].tolist(), hits["stringID"].tolist(), hits["omID"].tolist()))
        rows = list(zip(s, hits["pmt"].tolist(), hits["time"].view(np.uint64).tolist(), hits["id"].tolist()))
        return set(rows), len(rows)
    set_a, n_a = as_set(a[0], a[1])
    set_b, n_b = as_set(b[0], b[1])
    print(name, n_a, "hits,", n_b, "at half the collection efficiency")
    assert 0 < n_b < n_a and set_b < set_a
    # (as multisets too: the records are distinct, so neither set lost a member)
    assert len(set_a) == n_a and len(set_b) == n_b


def crafted():
    """(records, series, layout): aimed records with one of everything"""
    records, series, _ = Q.aimed_records(6000, 3)
    records, series = records.copy(), series.copy()
    functions, types, pmts, modules = Q.keep_all_layout()
    foreign = (modules["stringID"] == series["stringID"][2]) & (modules["omID"] == series["omID"][2])      # a module the generator does not have
    series["omID"][5] += 1                                                  # an entry naming another module than its records
    series[[7, 8]] = series[[8, 7]]                                         # `first` does not ascend: the bisection loses records
    records["weight"][np.arange(len(records)) % 97 == 5] = 1e6             # P > 1
    off = np.arange(len(records)) % 89 == 11                                # 10 cm off the sphere, along the position
    for k in ("x", "y", "z"):
        records[k][off] *= np.float32((PS.RADIUS + 0.10) / PS.RADIUS)
    return records, series, (functions, types, pmts, modules[~foreign])


def test_every_counter_counts():
    records, series, layout = crafted()
    got = PC.make_generator(*layout).MakeHitsFromFramePhotonsHost(records, series)
    print(got[2])
    assert all(got[2][k] > 0 for k in CV.PMT_PHOTON_HIT_COUNTERS), got[2]
    Q.same(got, Q.numpy_hits(records, series, *layout))
    # OFF_SURFACE records still make hits: a hit at every position that is off the sphere
    r2 = records["x"].astype(np.float64) ** 2 + records["y"].astype(np.float64) ** 2 + records["z"].astype(np.float64) ** 2
    off_times = set(records["time"][r2 > (PS.RADIUS + 0.05) ** 2].view(np.uint64).tolist())
    assert len(off_times & set(got[0]["time"].view(np.uint64).tolist())) > 10
    # an empty table: everything is UNCOVERED
    none = PC.make_generator(*layout).MakeHitsFromFramePhotonsHost(records, series[:0])
    assert len(none[0]) == 0 == len(none[1]) and none[2]["uncovered"] == len(records)


def test_properties_and_shuffling_within_the_series():
    layout = Q.keep_all_layout()
    gen = PC.make_generator(*layout)
    records, series, _ = Q.aimed_records(6000, 8, special_times=True)
    # exact copies among the records: equal keys, byte-identical hits
    records = records.copy()
    first, count = int(series["first"][3]), int(series["count"][3])
    assert count >= 4
    records[first + 1] = records[first]
    records[first + 3] = records[first + 2]
    got = gen.MakeHitsFromFramePhotonsHost(records, series)
    Q.check_properties(got[0], got[1], series)
    assert len(got[0]) == len(records)
    raw = got[0].view(np.uint8).reshape(len(got[0]), -1)
    assert int((raw[1:] == raw[:-1]).all(axis=1).sum()) >= 2
    shuffled = Q.shuffled_within_series(records, series, 4)
    assert shuffled.tobytes() != records.tobytes()
    Q.same(gen.MakeHitsFromFramePhotonsHost(shuffled, series), got)


def test_refusals():
    lib = _lib.load()
    gen = PC.make_generator(*Q.keep_all_layout())
    records, series, _ = Q.aimed_records(64, 2)
    out, out_series = np.zeros(64, dtype=CV.PMT_HIT_DTYPE), np.zeros(64, dtype=CV.PMT_SERIES_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n_kept, n_series = C.c_size_t(), C.c_size_t()
    call = lambda g, r, n, s, ns, o, os_: lib.clsimhip_pmt_photon_hits_host(g, r, n, s, ns, o, os_, C.byref(n_kept), C.byref(n_series), None)
    assert call(gen._h, vp(records), 64, vp(series), len(series), vp(out), vp(out_series)) == 0 and n_kept.value == 64
    # more than 2^26 series: by the argument alone (the table holds a few entries; nothing of it is read)
    assert call(gen._h, vp(records), 64, vp(series), (1 << 26) + 1, vp(out), vp(out_series)) == _lib.ERR_ARGUMENT
    assert b"2^26" in lib.clsimhip_pmt_generator_last_error(gen._h)
    # null pointers
    assert call(None, vp(records), 64, vp(series), len(series), vp(out), vp(out_series)) == _lib.ERR_ARGUMENT
    assert call(gen._h, None, 64, vp(series), len(series), vp(out), vp(out_series)) == _lib.ERR_ARGUMENT
    assert call(gen._h, vp(records), 64, None, len(series), vp(out), vp(out_series)) == _lib.ERR_ARGUMENT
    assert call(gen._h, vp(records), 64, vp(series), len(series), None, vp(out_series)) == _lib.ERR_ARGUMENT
    assert call(gen._h, vp(records), 64, vp(series), len(series), vp(out), None) == _lib.ERR_ARGUMENT
    # nothing to do needs no pointers
    assert call(gen._h, None, 0, None, 0, None, None) == 0 and n_kept.value == 0 == n_series.value
    # a generator of another kind has no such stage: the entry points take a clsimhip_pmt_generator, and only PMTHitGenerator has the methods
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert re.search(r"int clsimhip_pmt_photon_hits_host\(const clsimhip_pmt_generator \*g,", header)
    assert re.search(r"int clsimhip_pmt_photon_hits_device\(clsimhip_pmt_generator \*g,", header)
    for other in (CV.MCPEGenerator, CV.PhotonHitMaker, CV.FramePhotonDoms):
        assert not hasattr(other, "MakeHitsFromFramePhotonsHost") and not hasattr(other, "MakeHitsFromFramePhotonsDevice")
    # the device call's refusals that need no device: capacity beyond 2^26, a workspace that is too small, null and misaligned pointers
    a = 1 << 20     # (an address that is never read: every call below is refused before anything touches the device)
    big = CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(16)
    for args in ((a, a, a, (1 << 26) + 1, a, a, a, a, 1 << 40), (a, a, a, 16, a, a, a, a, big - 1), (0, a, a, 16, a, a, a, a, big), (a, 0, a, 16, a, a, a, a, big),
                 (a, a, 0, 16, a, a, a, a, big), (a, a, a, 16, 0, a, a, a, big), (a, a, a, 16, a, 0, a, a, big), (a, a, a, 16, a, a, 0, a, big),
                 (a, a, a, 16, a, a, a, 0, big), (a + 8, a, a, 16, a, a, a, a, big), (a, a + 8, a, 16, a, a, a, a, big), (a, a, a + 2, 16, a, a, a, a, big),
                 (a, a, a, 16, a + 8, a, a, a, big), (a, a, a, 16, a, a + 8, a, a, big), (a, a, a, 16, a, a, a + 2, a, big), (a, a, a, 16, a, a, a, a + 8, big)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            gen.MakeHitsFromFramePhotonsDevice(*args)
        assert e.value.code == _lib.ERR_ARGUMENT, args


def test_counters_and_layouts_are_the_headers():
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    for index, name in enumerate(CV.PMT_PHOTON_HIT_COUNTERS):
        assert re.search(r"#define CLSIMHIP_PMT_PHOTON_HITS_%s %d\b" % (name.upper(), index), header), name
    assert CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(1000) == CV.PhotonHitMaker.WorkspaceBytes(1000)        # one SeriesWorkspaceLayout


# ---- the stand-alone host program under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/pmt_photon_hits_host_main.cpp with clsim_amd/csrc/pmt_photon_hits.cpp and pmt_hits.cpp, host code only, with
    -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("pmt_photon_hits_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    sources = [os.path.join(ROOT, "clsim_amd", "csrc", "pmt_hits.cpp"), os.path.join(ROOT, "clsim_amd", "csrc", "pmt_photon_hits.cpp"),
               os.path.join(ROOT, "tests", "pmt_photon_hits_host_main.cpp")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c"] + sources, cwd=str(d))
    exe = str(d / "pmt_photon_hits_host_main")
    # (linked without the HIP runtime: the program defines the entry points the two files name)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "pmt_hits.o", "pmt_photon_hits.o",
                           "pmt_photon_hits_host_main.o", "-o", exe], cwd=str(d))
    return exe


def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path):
    cases = [(Q.fixture_records("mie"), PC.configuration("two_types", PC.sphere_radius_of("mie")))]
    records, series, layout = crafted()
    cases.append(((records, series), layout))
    cases.append(((records[:0], series[:0]), layout))
    for k, ((records, series), layout) in enumerate(cases):
        want = PC.make_generator(*layout).MakeHitsFromFramePhotonsHost(records, series)
        src, dst = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        Q.write_input(src, records, series, *layout)
        run = subprocess.run([host_program, src, dst], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stderr == "", run.stderr
        assert run.stdout.split() == ["kept", str(len(want[0])), "series", str(len(want[1])), "counters"] + [str(want[2][c]) for c in CV.PMT_PHOTON_HIT_COUNTERS]
        assert np.fromfile(dst, dtype=np.uint8).tobytes() == want[0].tobytes() + want[1].tobytes()
        assert k != 0 or len(want[0]) > 0
        assert k != 1 or all(v > 0 for v in want[2].values())
