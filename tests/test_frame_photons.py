"""Frame photons (include/clsimhip.h): the host twin (clsimhip_frame_photons_host) against an independent numpy restatement, byte
for byte; the properties of the output from the arrays alone; collisions of h and the bound on runs of colliding records; the struct
layout; and the twin as a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU here
(tests/test_frame_photons_gpu.py has the kernels)."""
import os
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import frame_photons_common as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
MASK = [(7, -3, 5), (2, 40, 60), (900, 86, 30), (11, 0, 5), (7, 3, 5), (7, 1, 25)]
same = F.same


def both(doms, photons, particles=None, masked=None):
    """the twin's result, checked against the restatement and for its properties"""
    got = doms.MakeFramePhotonsHost(photons, particles, masked)
    same(got, F.numpy_frame_photons(photons, F.DOM_STRINGS, F.DOM_OMS, particles, masked))
    F.check_properties(got[0], got[1])
    c = got[2]
    if not c["tie_overflow"]:
        assert len(got[0]) + c["masked"] + c["unknown_particle"] + c["unknown_dom"] == len(photons)
    return got


def test_twin_equals_the_restatement_on_quantised_times():
    doms = F.synthetic_doms()
    m = F.synthetic_photons(6000, seed=1)
    p = F.particle_table(m["id"])
    masked = F.mask_of(MASK)
    got = both(doms, m, p, masked)
    assert F.content_ties(got[0]) >= 50 and 0 < got[2]["masked"] < len(m) and len(set(got[1]["frame"])) == 3
    # exact copies are there too, and stay
    raw = got[0].view(np.uint8).reshape(len(got[0]), -1)
    assert (raw[1:] == raw[:-1]).all(axis=1).sum() >= 50
    # no table: one frame, 0, shift +0.0; no mask
    none = both(doms, m)
    assert (none[1]["frame"] == 0).all() and len(none[0]) == len(m) and F.content_ties(none[0]) >= 50
    # the same input shuffled: the same bytes
    rng = np.random.default_rng(9)
    for _ in range(3):
        same(doms.MakeFramePhotonsHost(m[rng.permutation(len(m))], p, masked), got)
    # an empty table is a table: every identifier is unknown
    empty = both(doms, m, np.zeros(0, dtype=CV.MCPE_PARTICLE_DTYPE))
    assert empty[2]["unknown_particle"] == len(m) and len(empty[0]) == 0
    # unknown identifiers through the binary search (gaps) and the offset form (consecutive), unknown DOMs
    every = np.unique(m["id"])
    for ids in (every[::2], every[5:25]):
        assert both(doms, m, F.particle_table(ids))[2]["unknown_particle"] > 0
    odd = m.copy()
    odd["stringID"][:10] = 17
    assert both(doms, odd, p, masked)[2]["unknown_dom"] == 10


def test_special_times_keep_their_bits_and_their_order():
    doms = F.synthetic_doms()
    m = F.synthetic_photons(4000, seed=2)
    assert set(F.SPECIAL_TIMES.view(np.uint32).tolist()) <= set(m["t"].view(np.uint32).tolist())
    got = both(doms, m)
    bits = set(got[0]["time"].view(np.uint64).tolist())
    # +0.0 and -0.0 both arrive as +0.0 (the shift is +0.0); the infinities and both NaNs, widened, payload kept
    assert {0x0, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000020000000} <= bits and 0x8000000000000000 not in bits
    p = F.particle_table(m["id"], frames=(3,))
    p["timeShift"] = -0.0
    assert 0x8000000000000000 in set(both(doms, m, p)[0]["time"].view(np.uint64).tolist())


def test_shifts_that_round_distinct_times_onto_one_value():
    doms = F.synthetic_doms()
    m = F.synthetic_photons(3000, seed=3, special=False, quantised=False)
    m["stringID"], m["omID"] = 1, 25
    m["id"] = 1000 + np.arange(len(m)) % 2
    p = F.particle_table(m["id"], frames=(5,))
    p["timeShift"] = 2.0 ** 70                           # (one ulp there is 2^18 ns) every time of the bunch becomes 2^70
    assert len(set(m["t"].tolist())) > 2000
    got = both(doms, m, p)
    assert set(got[0]["time"].tolist()) == {2.0 ** 70} and len(got[1]) == 1 and F.content_ties(got[0]) >= 50
    assert (np.diff(got[0]["id"].astype(np.int64)) >= 0).all()           # one (group, tkey): the identifier decides first


def test_collisions_of_h_and_the_bound():
    a, b = F.colliding_pair()
    assert (a != b).any() and F.mix(a)[0] == F.mix(b)[0]
    doms = F.synthetic_doms()
    for length in (2, 65, 2048):
        got = both(doms, F.collision_run(length, seed=40 + length))
        assert got[2]["tie_overflow"] == 0 and len(got[0]) == 200 + length
        run = got[0][(got[0]["id"] == 1003) & (got[0]["time"] == 1234.5) & (got[0]["stringID"] == 1) & (got[0]["omID"] == 25)]
        w = F.words_of(run)
        first_b = int(np.flatnonzero((w != w[0]).any(axis=1))[0])
        assert len(run) == length and 0 < first_b < length
        assert (w[:first_b] == w[0]).all() and (w[first_b:] == w[-1]).all() and len(set(F.mix(w).tolist())) == 1
    got = both(doms, F.collision_run(2049, seed=44))
    assert got[2]["tie_overflow"] == 2049 and len(got[0]) == 0 and len(got[1]) == 0
    got = both(doms, F.collision_run(5000, seed=45, only_a=True))
    assert got[2]["tie_overflow"] == 0 and len(got[0]) == 5200


def test_bad_tables_and_ids_are_refused():
    doms = F.synthetic_doms()
    m = F.synthetic_photons(100, seed=4)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="strictly increasing") as e:
        doms.MakeFramePhotonsHost(m, F.particle_table(m["id"])[::-1])
    assert e.value.code == _lib.ERR_ARGUMENT
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="does not fit the photon record") as e:
        CV.FramePhotonDoms([1, 40000], [1, 2])
    assert e.value.code == _lib.ERR_ARGUMENT
    # a pair named twice is one DOM; no DOM at all: every record is UNKNOWN_DOM
    twice = CV.FramePhotonDoms(np.concatenate([F.DOM_STRINGS, F.DOM_STRINGS[:5]]), np.concatenate([F.DOM_OMS, F.DOM_OMS[:5]]))
    same(twice.MakeFramePhotonsHost(m), doms.MakeFramePhotonsHost(m))
    assert CV.FramePhotonDoms([], []).MakeFramePhotonsHost(m)[2]["unknown_dom"] == len(m)


def test_struct_layout_matches_the_header(tmp_path):
    members = ["identifier", "string_id", "om_id", "time", "weight", "wavelength", "group_velocity", "x", "y", "z", "theta", "phi"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "clsimhip.h"', "int main(void) {", 'printf("%zu\\n", sizeof(clsimhip_frame_photon));']
    lines += ['printf("%%zu\\n", offsetof(clsimhip_frame_photon, %s));' % k for k in members]
    lines += ['printf("%d %d %d %d %d\\n", CLSIMHIP_FRAME_PHOTONS_UNKNOWN_PARTICLE, CLSIMHIP_FRAME_PHOTONS_MASKED, CLSIMHIP_FRAME_PHOTONS_UNKNOWN_DOM, '
              'CLSIMHIP_FRAME_PHOTONS_TIE_OVERFLOW, CLSIMHIP_FRAME_PHOTONS_TIE_BOUND);', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    words = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    dtype = CV.FRAME_PHOTON_DTYPE
    assert len(dtype.names) == len(members) and dtype.itemsize == 48
    assert words == [48] + [dtype.fields[k][1] for k in dtype.names] + [CV.FRAME_PHOTON_COUNTERS.index(k) for k in
                                                                        ("unknown_particle", "masked", "unknown_dom", "tie_overflow")] + [F.BOUND]
    assert CV.FRAME_PHOTON_TIE_BOUND == F.BOUND


# ---- the twin as a program of its own, under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/frame_photons_host_main.cpp with clsim_amd/csrc/frame_photons.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("frame_photons_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    sources = [os.path.join(ROOT, "clsim_amd", "csrc", "frame_photons.cpp"), os.path.join(ROOT, "tests", "frame_photons_host_main.cpp")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c"] + sources, cwd=str(d))
    exe = str(d / "frame_photons_host_main")
    # (linked without the HIP runtime: the program defines the entry points the file names)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "frame_photons.o",
                           "frame_photons_host_main.o", "-o", exe], cwd=str(d))
    return exe


def run_host_program(exe, tmp_path, photons, particles, masked):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    have_table = particles is not None
    p = np.ascontiguousarray(particles if have_table else [], dtype=CV.MCPE_PARTICLE_DTYPE)
    k = np.ascontiguousarray(masked if masked is not None else [], dtype=CV.MCPE_MASK_DTYPE)
    with open(src, "wb") as f:
        f.write(np.array([len(F.DOM_STRINGS), len(photons), len(p), len(k), int(have_table)], dtype=np.uint64).tobytes())
        f.write(F.DOM_STRINGS.astype(np.int32).tobytes() + F.DOM_OMS.astype(np.uint32).tobytes())
        f.write(np.ascontiguousarray(photons, dtype=CV.PHOTON_DTYPE).tobytes() + p.tobytes() + k.tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    return run, (np.fromfile(dst, dtype=np.uint8) if run.returncode == 0 else None)


def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path):
    doms = F.synthetic_doms()
    cases = [(F.synthetic_photons(3000, seed=6), "table", F.mask_of(MASK)), (F.synthetic_photons(500, seed=7), None, None),
             (F.synthetic_photons(0, seed=8), None, None), (F.collision_run(2048, seed=46), None, None), (F.collision_run(2049, seed=47), None, None)]
    for m, table, masked in cases:
        p = F.particle_table(m["id"]) if table else None
        want = doms.MakeFramePhotonsHost(m, p, masked)
        run, out = run_host_program(host_program, tmp_path, m, p, masked)
        assert run.returncode == 0 and not run.stderr, run.stderr
        c = want[2]
        assert run.stdout.split() == ["kept", str(len(want[0])), "series", str(len(want[1])), "counters", str(c["unknown_particle"]), str(c["masked"]),
                                      str(c["unknown_dom"]), str(c["tie_overflow"])]
        assert out.tobytes() == want[0].tobytes() + want[1].tobytes()
    # a table that does not increase: an error message and exit code 1, not a crash
    m = cases[0][0]
    run, _ = run_host_program(host_program, tmp_path, m, F.particle_table(m["id"])[::-1], None)
    assert run.returncode == 1 and "strictly increasing" in run.stderr
