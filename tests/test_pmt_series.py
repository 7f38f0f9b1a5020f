"""PMT series, host side: the host twin (clsimhip_pmt_series_host) against an independent numpy restatement of the definition
(tests/pmt_series_common.py), byte for byte, on the hit maker's hits of the committed fixtures in the three configurations of
tests/pmt_common.py and on synthetic hits; the properties of the output; the refusals; the record layouts; the stand-alone host
program under AddressSanitizer and UndefinedBehaviorSanitizer.  Every test asserts that its input contains what it claims to
cover.  No GPU here (tests/test_pmt_series_gpu.py has the kernels, and the setter's refusal after Initialize(), which needs one)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import mcpe_common as M
from tests import pmt_common as PC
from tests import pmt_series_common as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CASES = [(name, cfg) for name in PC.FIXTURES for cfg in PC.CONFIGURATIONS]
same = PS.same


def refused(code, call, text):
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=text) as e:
        call()
    assert e.value.code == code, str(e.value)


@pytest.mark.parametrize("name,cfg", CASES)
def test_twin_equals_numpy_on_the_fixtures(name, cfg):
    functions, types, pmts, modules = PC.configuration(cfg, PC.sphere_radius_of(name))
    gen = PC.make_generator(functions, types, pmts, modules)
    hits, _ = gen.ConvertHost(M.fixture_photons(name))
    assert len(hits) > 0
    # no table: one frame, 0
    got = gen.MakeSeriesHost(hits)
    same(got, PS.numpy_series(hits, types, modules))
    PS.check_properties(got[0], got[1])
    assert len(got[0]) == len(hits) and (got[1]["frame"] == 0).all()
    assert PC.sort_hits(got[0]).tobytes() == PC.sort_hits(hits).tobytes()          # the same records, in another order
    # three frames with interleaved identifiers (one frame when the fixture has a single identifier), shifts, a mask
    p = PS.particle_table(hits["id"])
    codes = PS.module_code(hits["stringID"], hits["omID"])
    busiest = np.bincount(codes).argmax()
    sid, oid = busiest // 65536 - 32768, busiest % 65536
    masked = PS.mask_of([(f, sid, oid) for f in (7, 2, 900)] + [(5, sid, oid), (7, 99, 99)])
    got = gen.MakeSeriesHost(hits, p, masked)
    same(got, PS.numpy_series(hits, types, modules, p, masked))
    PS.check_properties(got[0], got[1])
    assert 0 < got[2]["masked"] and (got[2]["masked"] < len(hits) or len(np.unique(codes)) == 1)
    assert set(got[1]["frame"]) <= {7, 2, 900} and got[2]["unknown_particle"] == 0 == got[2]["unknown_channel"]
    assert not ((got[0]["stringID"] == sid) & (got[0]["omID"] == oid)).any()


def test_twin_equals_numpy_on_synthetic_hits():
    gen, types, modules = PS.synthetic_generator()
    h = PS.synthetic_hits(20000, seed=1)
    p = PS.particle_table(h["id"])
    masked = PS.mask_of([(7, -3, 5), (2, 40, 60), (900, 86, 30), (11, 0, 5), (7, 3, 5)])
    # what this input covers
    assert len(set(p["frame"])) == 3 and len(p) >= 9 and list(p["frame"][:6]) == [7, 2, 900, 7, 2, 900]             # interleaved identifiers
    assert (h["stringID"] < 0).any() and (h["pmt"] == 63).any() and (h["pmt"][h["stringID"] % 2 == 0] <= 30).all()
    assert PS.SPECIAL_BITS <= set(h["time"].view(np.uint64).tolist())
    assert len(set(types["numPMTs"])) == 2 and len(set(modules["type"])) == 2
    got = gen.MakeSeriesHost(h, p, masked)
    same(got, PS.numpy_series(h, types, modules, p, masked))
    PS.check_properties(got[0], got[1])
    records, series, counters = got
    assert 0 < counters["masked"] < len(h) and len(records) == len(h) - counters["masked"]
    # a masked module loses all its PMTs, in the masked frame only
    frame_of = dict(zip(p["id"].tolist(), p["frame"].tolist()))
    at_module = (h["stringID"] == -3) & (h["omID"] == 5)
    in_frame = np.array([frame_of[i] == 7 for i in h["id"][at_module].tolist()])
    assert len(set(h["pmt"][at_module][in_frame].tolist())) > 5
    assert not ((series["frame"] == 7) & (series["stringID"] == -3) & (series["omID"] == 5)).any()
    assert ((series["frame"] == 2) & (series["stringID"] == -3) & (series["omID"] == 5)).any()
    # records with equal time' and different identifiers, ascending in the identifier
    t = PS.tkey_of(records["time"])
    owner = np.repeat(np.arange(len(series)), series["count"])
    tie = (owner[1:] == owner[:-1]) & (t[1:] == t[:-1])
    assert (tie & (records["id"][1:] != records["id"][:-1])).sum() > 0
    # frames come out in ascending frame ID, whatever the table's order of frames
    assert list(np.unique(series["frame"])) == [2, 7, 900] and (np.diff(series["frame"].astype(np.int64)) >= 0).all()


def test_a_shift_of_minus_zero_keeps_every_bit_pattern():
    """the total order on bit patterns: in a series, -NaN < -inf < -0.0 < +0.0 < +inf < +NaN.  With a shift of -0.0 every time keeps
    its bits (+0.0, the no-table default, turns -0.0 into +0.0: it is an addition)"""
    gen, types, modules = PS.synthetic_generator()
    h = PS.synthetic_hits(20000, seed=1)
    h["stringID"][:3000], h["omID"][:3000], h["pmt"][:3000] = 1, 25, 63           # one long series with several of the special times
    h["time"][:48] = np.tile(PS.SPECIAL_TIMES, 4)
    p0 = PS.particle_table(h["id"], frames=(3,))
    p0["timeShift"] = -0.0
    got = gen.MakeSeriesHost(h, p0)
    same(got, PS.numpy_series(h, types, modules, p0))
    PS.check_properties(got[0], got[1])
    assert PC.sort_hits(got[0]).tobytes() == PC.sort_hits(h).tobytes()
    bits = got[0]["time"].view(np.uint64)
    order = (0xFFF8000000000001, 0xFFF0000000000000, 0x8000000000000000, 0x0, 0x7FF0000000000000, 0x7FF8000000000000)
    full = 0
    for first, count in zip(got[1]["first"], got[1]["count"]):
        inside = bits[first:first + count].tolist()
        position = {v: inside.index(v) for v in order if v in inside}
        assert list(position.values()) == sorted(position.values())
        full += len(position) == len(order)
    assert full >= 1
    # without a table the shift is +0.0
    plain = gen.MakeSeriesHost(h)
    assert not (plain[0]["time"].view(np.uint64) == 0x8000000000000000).any() and (bits == 0x8000000000000000).any()


def test_output_does_not_depend_on_the_input_order():
    gen, types, modules = PS.synthetic_generator()
    h = PS.synthetic_hits(5000, seed=2)
    p = PS.particle_table(h["id"])
    masked = PS.mask_of([(2, 1, 10)])
    base = gen.MakeSeriesHost(h, p, masked)
    rng = np.random.default_rng(5)
    for _ in range(4):
        same(gen.MakeSeriesHost(h[rng.permutation(len(h))], p, masked), base)
    same(gen.MakeSeriesHost(h[::-1], p, masked[::-1]), base)


def test_empty_and_single_inputs():
    gen, types, modules = PS.synthetic_generator()
    for n in (0, 1):
        h = PS.synthetic_hits(n, seed=4, special=False)
        for p in (None, PS.particle_table([1000 + k for k in range(40)])):
            got = gen.MakeSeriesHost(h, p)
            same(got, PS.numpy_series(h, types, modules, p))
            assert len(got[0]) == n and len(got[1]) == n
    # a mask that removes the only record
    h = PS.synthetic_hits(1, seed=4, special=False)
    got = gen.MakeSeriesHost(h, None, PS.mask_of([(0, int(h["stringID"][0]), int(h["omID"][0]))]))
    assert len(got[0]) == 0 and len(got[1]) == 0 and got[2]["masked"] == 1


def test_unknown_identifiers_are_counted_and_dropped():
    gen, types, modules = PS.synthetic_generator()
    h = PS.synthetic_hits(3000, seed=6)
    every = np.unique(h["id"])
    # a table with gaps (the binary search) and one without (the offset form): the same definition
    for ids in (every[::2], every[5:25]):
        p = PS.particle_table(ids)
        got = gen.MakeSeriesHost(h, p)
        same(got, PS.numpy_series(h, types, modules, p))
        unknown = int((~np.isin(h["id"], ids)).sum())
        assert got[2]["unknown_particle"] == unknown > 0 and len(got[0]) == len(h) - unknown > 0
    assert np.all(np.diff(every[5:25].astype(np.int64)) == 1) and not np.all(np.diff(every[::2].astype(np.int64)) == 1)
    # an empty table knows nobody
    got = gen.MakeSeriesHost(h, np.zeros(0, dtype=CV.MCPE_PARTICLE_DTYPE))
    assert got[2]["unknown_particle"] == len(h) and len(got[0]) == 0


def test_unknown_channels_are_counted_both_ways():
    gen, types, modules = PS.synthetic_generator()
    h = PS.synthetic_hits(3000, seed=6)
    p = PS.particle_table(np.unique(h["id"])[3:])   # (some of the unknown channels have unknown particles too: the channel comes first)
    # a module the generator lacks
    h["stringID"][:10] = 17
    h["id"][:2] = np.unique(h["id"])[:2]
    # pmt = the type's n_pmts: 31 on an even string, 64 on an odd one; 63 on an odd string stays
    even, odd = np.flatnonzero(h["stringID"] % 2 == 0)[:7], np.flatnonzero(h["stringID"] == 1)[:5]
    h["pmt"][even], h["pmt"][odd[:3]], h["pmt"][odd[3:]] = 31, 64, 63
    got = gen.MakeSeriesHost(h, p)
    same(got, PS.numpy_series(h, types, modules, p))
    assert got[2]["unknown_channel"] == 10 + 7 + 3 and got[2]["unknown_particle"] > 0
    assert (~np.isin(h["id"][:10], p["id"])).any() and len(got[0]) + 20 + got[2]["unknown_particle"] == len(h)
    assert (got[0]["pmt"] == 63).any() and not (got[0]["stringID"] == 17).any()
    # a generator without modules has no channel at all
    functions, types, pmts, modules = PS.synthetic_layout()
    none = PC.make_generator(functions, types, pmts, modules[:0])
    got = none.MakeSeriesHost(h)
    assert got[2]["unknown_channel"] == len(h) and len(got[0]) == 0 == len(got[1])


def test_a_masked_module_loses_all_its_pmts():
    gen, types, modules = PS.synthetic_generator()
    h = PS.synthetic_hits(4000, seed=8)
    at = (h["stringID"] == 2) & (h["omID"] == 15)
    assert len(set(h["pmt"][at].tolist())) > 3
    hidden = gen.MakeSeriesHost(h, None, PS.mask_of([(0, 2, 15), (1, 2, 20)]))                 # frame 0's mask applies, another frame's does not
    same(hidden, PS.numpy_series(h, types, modules, None, PS.mask_of([(0, 2, 15), (1, 2, 20)])))
    assert 0 < hidden[2]["masked"] == int(at.sum()) < len(h)
    assert not ((hidden[0]["stringID"] == 2) & (hidden[0]["omID"] == 15)).any() and ((hidden[0]["stringID"] == 2) & (hidden[0]["omID"] == 20)).any()


def test_a_table_that_is_not_strictly_increasing_is_refused():
    gen, _, _ = PS.synthetic_generator()
    h = PS.synthetic_hits(100, seed=7, special=False)
    for order in ([1000, 1002, 1001], [1000, 1001, 1001]):
        p = np.zeros(3, dtype=CV.MCPE_PARTICLE_DTYPE)
        p["id"] = order
        refused(_lib.ERR_ARGUMENT, lambda: gen.MakeSeriesHost(h, p), "strictly increasing")


def test_frames_times_channels_beyond_32_bits_is_refused():
    """65 536 modules of 64 PMTs are 2^22 channels: 1 024 frames are too many, 1 023 are taken"""
    functions, types, pmts, _ = PS.synthetic_layout()
    strings = np.arange(-32768, 32768, dtype=np.int32)
    modules = np.zeros(len(strings), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"], modules["type"] = strings, 1, 1
    modules["rotation"] = np.eye(3).reshape(9)
    gen = PC.make_generator(functions, types, pmts, modules)
    h = np.zeros(4, dtype=CV.PMT_HIT_DTYPE)
    h["id"], h["stringID"], h["omID"], h["pmt"], h["time"] = [5, 1023, 0, 5], [-32768, 32767, 0, -32768], 1, [0, 63, 7, 0], [3.0, 2.0, 1.0, 1.5]
    p = np.zeros(1024, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"] = np.arange(1024)
    p["frame"] = np.arange(1024)[::-1] * 3
    refused(_lib.ERR_CONFIG, lambda: gen.MakeSeriesHost(h, p), "do not fit 32 bits")
    got = gen.MakeSeriesHost(h, p[:1023])          # 1 023 frames x 2^22 channels: the largest group index is 2^32 - 2^22 - 1
    same(got, PS.numpy_series(h, types, modules, p[:1023]))
    assert got[2]["unknown_particle"] == 1 and list(got[0]["id"]) == [5, 5, 0]


def test_workspace_query_and_compile_refusals():
    assert CV.PMTHitGenerator.SeriesWorkspaceBytes(1 << 20) >= 2 * 16 * (1 << 20)
    assert CV.PMTHitGenerator.SeriesWorkspaceBytes(1 << 20, 1000, 10) > CV.PMTHitGenerator.SeriesWorkspaceBytes(1 << 20)
    assert CV.PMTHitGenerator.SeriesWorkspaceBytes(0) > 0
    # the switch is a configuration call: before Initialize() it needs no GPU, and Compile() wants a PMT hit generator with it
    from tests import common
    cfg = common.config("c1")
    conv = common.product_converter(cfg, 512, initialize=False)
    conv.SetPMTSeries(True)
    refused(_lib.ERR_CONFIG, conv.Compile, "need a PMT hit generator")
    g = cfg["geom"]
    s, d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    conv.SetMCPEGenerator(M.make_generator([M.acceptance_table()], s, d, np.zeros(len(s), dtype=np.int32)), True)
    refused(_lib.ERR_CONFIG, conv.Compile, "need a PMT hit generator")                        # an MCPE generator is not one
    conv.SetMCPEGenerator(None)
    conv.SetPMTHitGenerator(PC.geometry_generator(cfg), True)
    conv.Compile()
    conv.SetMCPESeries(True)                                                                    # the MCPE switch stays refused beside a PMT generator
    refused(_lib.ERR_CONFIG, conv.Compile, "MCPE series")
    conv.SetMCPESeries(False)
    conv.SetPMTSeries(False)
    conv.SetPMTHitGenerator(None)
    conv.Compile()


def test_records_match_the_header(tmp_path):
    """24-byte series entries; every field sits where the numpy dtype puts it (include/clsimhip.h compiled as C99)"""
    assert CV.PMT_SERIES_DTYPE.itemsize == 24 == CV.PMT_HIT_DTYPE.itemsize
    members = ["frame", "string_id", "om_id", "pmt", "first", "count", "reserved"]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "clsimhip.h"', "int main(void) {", 'printf("%zu", sizeof(clsimhip_pmt_series));']
    lines += ['printf(" %%zu", offsetof(clsimhip_pmt_series, %s));' % member for member in members]
    lines.append('printf(" %d %d %d\\n", CLSIMHIP_PMT_SERIES_UNKNOWN_PARTICLE, CLSIMHIP_PMT_SERIES_MASKED, CLSIMHIP_PMT_SERIES_UNKNOWN_CHANNEL);')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    words = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    dtype = CV.PMT_SERIES_DTYPE
    assert len(dtype.names) == len(members)
    assert words == [dtype.itemsize] + [dtype.fields[k][1] for k in dtype.names] + [CV.PMT_SERIES_COUNTERS.index(k) for k in ("unknown_particle", "masked", "unknown_channel")]
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert re.search(r"sizeof\(clsimhip_pmt_series\) == 24 \? 1 : -1", header)


# ---- the stand-alone host program under the sanitizers ----
def write_input(path, hits, functions, types, pmts, modules, particles, masked):
    have_table = particles is not None
    particles = np.zeros(0, dtype=CV.MCPE_PARTICLE_DTYPE) if particles is None else np.ascontiguousarray(particles, dtype=CV.MCPE_PARTICLE_DTYPE)
    masked = np.zeros(0, dtype=CV.MCPE_MASK_DTYPE) if masked is None else np.ascontiguousarray(masked, dtype=CV.MCPE_MASK_DTYPE)
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", len(functions), len(types), len(pmts), len(modules), len(hits), len(particles), len(masked), int(have_table)))
        for fn in functions:
            if fn[0] == "table":
                f.write(struct.pack("<2q3d", 0, len(fn[3]), fn[1], fn[2], 0.0))
                f.write(np.asarray(fn[3], dtype="<f8").tobytes())
            else:
                f.write(struct.pack("<2q3d", 1, 0, 0.0, 0.0, fn[1]))
        for array in (types, pmts, modules, hits, particles, masked):
            f.write(np.ascontiguousarray(array).tobytes())


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/pmt_series_host_main.cpp with clsim_amd/csrc/pmt_series.cpp and pmt_hits.cpp, host code only, with
    -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("pmt_series_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    sources = [os.path.join(ROOT, "clsim_amd", "csrc", "pmt_hits.cpp"), os.path.join(ROOT, "clsim_amd", "csrc", "pmt_series.cpp"),
               os.path.join(ROOT, "tests", "pmt_series_host_main.cpp")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c"] + sources, cwd=str(d))
    exe = str(d / "pmt_series_host_main")
    # (linked without the HIP runtime: the program defines the entry points the two files name)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "pmt_hits.o", "pmt_series.o",
                           "pmt_series_host_main.o", "-o", exe], cwd=str(d))
    return exe


def run_host_program(exe, tmp_path, hits, layout, particles, masked):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(src, hits, *layout, particles, masked)
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    return run, (np.fromfile(dst, dtype=np.uint8) if run.returncode == 0 else None)


def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path):
    layout = PS.synthetic_layout()
    gen = PC.make_generator(*layout)
    h = PS.synthetic_hits(20000, seed=1)
    h["stringID"][:10] = 17
    h["pmt"][np.flatnonzero(h["stringID"] % 2 == 0)[:7]] = 31
    p = PS.particle_table(np.unique(h["id"])[::2])
    masked = PS.mask_of([(7, -3, 5), (2, 40, 60), (900, 86, 30), (11, 0, 5), (7, 3, 5)])
    assert PS.SPECIAL_BITS <= set(h["time"].view(np.uint64).tolist())
    for particles, mask in ((p, masked), (None, None), (p[:0], masked), (None, masked)):
        want = gen.MakeSeriesHost(h, particles, mask)
        run, out = run_host_program(host_program, tmp_path, h, layout, particles, mask)
        assert run.returncode == 0 and run.stderr == "", run.stderr
        assert run.stdout.split() == ["kept", str(len(want[0])), "series", str(len(want[1])), "counters"] + [str(want[2][k]) for k in CV.PMT_SERIES_COUNTERS]
        assert out.tobytes() == want[0].tobytes() + want[1].tobytes()
    assert all(v > 0 for v in gen.MakeSeriesHost(h, p, masked)[2].values())
    # n = 0; and a refused table is an error message and a status, nothing the sanitizers report
    run, out = run_host_program(host_program, tmp_path, h[:0], layout, p, masked)
    assert run.returncode == 0 and run.stderr == "" and len(out) == 0
    run, _ = run_host_program(host_program, tmp_path, h[:10], layout, p[::-1], masked)
    assert run.returncode == 1 and "strictly increasing" in run.stderr and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
