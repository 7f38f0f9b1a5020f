"""Multi-PMT hit generator, host side: the host twin (clsimhip_pmt_convert_host) against an independent numpy restatement of the
definition in include/clsimhip.h on the committed photon records of six configurations and one synthetic 31-PMT layout
(tests/pmt_common.py); the three condition counters; the refusals of create and of Compile(); the stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU here (tests/test_pmt_hits_gpu.py has the kernel)."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import mcpe_common as M
from tests import pmt_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CASES = [(name, cfg) for name in PC.FIXTURES for cfg in PC.CONFIGURATIONS]


@functools.lru_cache(maxsize=None)
def reference(name, cfg):
    """(photons, configuration, numpy hits, numpy counters, details), computed once and left as it is"""
    ph = M.fixture_photons(name)
    configuration = PC.configuration(cfg, PC.sphere_radius_of(name))
    return (ph, configuration) + PC.numpy_pmt_hits(ph, *configuration)


def counters_of(**kw):
    return dict(dict.fromkeys(CV.PMT_CONDITIONS, 0), **kw)


def refused(code, call):
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("name,cfg", CASES)
def test_host_twin_equals_numpy_restatement(name, cfg):
    ph, configuration, want, want_counters, details = reference(name, cfg)
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    assert counters == want_counters == counters_of()
    assert len(got) == len(want) > 0
    assert got.tobytes() == want.tobytes()              # same records, same order, same bits
    assert np.array_equal(got["time"], ph["t"][details["accepted"]].astype(np.float64)) and not got["reserved"].any()


def test_the_layout_exercises_the_closest_intersection_rule():
    """no record is leaving; more than half of every fixture's records find a PMT; every fixture but the smallest holds records
    that meet two discs (all of them together do, too); the larger fixtures use all 31 PMTs"""
    doubles = 0
    for name in PC.FIXTURES:
        ph, _, _, _, details = reference(name, "identity")
        found, double = details["found"] >= 0, details["double"]
        print("%s: %d of %d records find a PMT, %d meet two discs, %d PMTs used" % (name, found.sum(), len(ph), double.sum(), len(np.unique(details["found"][found]))))
        assert details["entering"].all() and 2 * found.sum() > len(ph)
        assert name == "c1" or double.sum() >= 1
        assert name == "c1" or len(np.unique(details["found"][found])) == 31
        doubles += int(double.sum())
    assert doubles >= 1


@pytest.mark.parametrize("name", PC.FIXTURES)
def test_a_rotated_module_sees_other_hits(name):
    plain, tilted = reference(name, "identity")[2], reference(name, "tilted")[2]
    assert plain.tobytes() != tilted.tobytes()
    assert not np.array_equal(reference(name, "identity")[4]["found"], reference(name, "tilted")[4]["found"])


@pytest.mark.parametrize("name", ["mie", "lea", "mie_60_keep", "lea_no_pancake"])
def test_two_types_by_string_parity(name):
    """odd strings carry the 4-PMT type with another quantum efficiency: their hits name PMTs 0 ... 3, and they are not the hits
    the 31-PMT type makes there"""
    ph, _, hits, _, details = reference(name, "two_types")
    odd = hits["stringID"] % 2 == 1
    assert odd.any() and (~odd).any() and hits["pmt"][odd].max() <= 3 and hits["pmt"][~odd].max() > 3
    one = reference(name, "identity")[2]
    assert one[one["stringID"] % 2 == 0].tobytes() == hits[~odd].tobytes()
    assert one[one["stringID"] % 2 == 1].tobytes() != hits[odd].tobytes()


@pytest.mark.parametrize("name,cfg", CASES)
def test_accepted_count_follows_the_probabilities(name, cfg):
    """accepted count > 0 and within 4 binomial sigma of the sum of P over the records that reach the draw"""
    _, _, hits, _, details = reference(name, cfg)
    P = details["P"][details["drawn"]]
    assert len(P) > 0 and 0.0 < P.min() and P.max() < 1.0
    sigma = np.sqrt(np.sum(P * (1.0 - P)))
    print("%s %s: accepted %d, sum P %.1f, sigma %.2f" % (name, cfg, len(hits), P.sum(), sigma))
    assert len(hits) > 0 and abs(len(hits) - P.sum()) < 4.0 * sigma


def test_draw_depends_on_the_seed_and_not_on_the_order():
    ph, configuration = reference("mie", "identity")[:2]
    a, _ = PC.make_generator(*configuration, seed=1).ConvertHost(ph)
    b, _ = PC.make_generator(*configuration, seed=2).ConvertHost(ph)
    assert a.tobytes() != b.tobytes()
    order = np.random.default_rng(5).permutation(len(ph))
    c, _ = PC.make_generator(*configuration, seed=1).ConvertHost(ph[order])
    assert PC.sort_hits(c).tobytes() == PC.sort_hits(a).tobytes()


def doctored():
    """(photons, configuration): records of `mie` and -- against R = 0.1651 m -- of `lea_no_pancake`, string 40 without a module,
    and a quantum efficiency scaled so that some P exceed 1"""
    ph = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea_no_pancake")])
    strings = [s for s in range(86) if s != 40]
    return ph, PC.configuration("two_types", PC.sphere_radius_of("mie"), q_scale=1.8, strings=strings)


def test_condition_counters_equal_the_restatement_on_a_doctored_input():
    ph, configuration = doctored()
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    want, want_counters, details = PC.numpy_pmt_hits(ph, *configuration)
    print(counters)
    assert counters == want_counters and all(v > 0 for v in counters.values())
    assert counters["unknown_module"] == int((ph["stringID"] == 40).sum())
    assert got.tobytes() == want.tobytes() and len(got) > 0


def test_records_off_the_surface_are_counted_and_still_processed():
    """records taken at r = 0.8255 m against a type of R = 0.1651 m: every one is counted, and those whose ray meets a disc go on
    to the draw like any other"""
    ph = M.fixture_photons("lea_no_pancake")
    configuration = PC.configuration("identity", PC.sphere_radius_of("mie"))
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    want, want_counters, details = PC.numpy_pmt_hits(ph, *configuration)
    assert counters == want_counters == counters_of(off_surface=len(ph))
    assert (details["found"] >= 0).sum() > 0 and details["drawn"].sum() > 0
    assert got.tobytes() == want.tobytes()


def test_a_removed_string_is_an_unknown_module():
    ph = M.fixture_photons("mie")
    gone = int(ph["stringID"][0])
    configuration = PC.configuration("identity", PC.sphere_radius_of("mie"), strings=[s for s in range(86) if s != gone])
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    want, want_counters, _ = PC.numpy_pmt_hits(ph, *configuration)
    assert counters == want_counters == counters_of(unknown_module=int((ph["stringID"] == gone).sum()))
    assert got.tobytes() == want.tobytes() and not (got["stringID"] == gone).any()


def test_probability_above_one_is_counted():
    ph = M.fixture_photons("mie")
    configuration = PC.configuration("identity", PC.sphere_radius_of("mie"), q_scale=2.0)
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    want, want_counters, _ = PC.numpy_pmt_hits(ph, *configuration)
    assert counters == want_counters == counters_of(probability_above_one=counters["probability_above_one"])
    assert counters["probability_above_one"] > 0 and got.tobytes() == want.tobytes()


def grazing_disc(side):
    """One record and one disc built around it.  The record's direction is edited to run 0.3 inwards and 1 along the sphere; the
    disc's axis is perpendicular to that direction up to n . d = side x 5e-9 (angles are binary32: no direction can be turned to
    within 1e-8 of a given plane, so the plane is turned to the direction), and its centre lies 2 cm down the ray, so that the ray
    meets the disc's plane 0.2 mm ahead, inside the disc.  side = +1: from behind (0 <= d . n < 1e-8, c <= 0); -1: from the front."""
    ph = M.fixture_photons("mie")[:1].copy()
    p = np.array([ph["x"][0], ph["y"][0], ph["z"][0]], dtype=np.float64)
    radial = p / np.sqrt(p @ p)
    along = np.cross(radial, [0.0, 0.0, 1.0])
    along /= np.sqrt(along @ along)
    d = -0.3 * radial + along
    d /= np.sqrt(d @ d)
    ph["theta"] = np.float32(np.arccos(d[2]))
    ph["phi"] = np.float32(np.arctan2(d[1], d[0]) % (2.0 * np.pi))
    st, ct = (float(M.capi.eval_math(k, ph["theta"])[0]) for k in (2, 3))
    sp, cp = (float(M.capi.eval_math(k, ph["phi"])[0]) for k in (2, 3))
    d = np.array([st * cp, st * sp, ct])                # the direction the hit maker will compute
    across = p - (p @ d) / (d @ d) * d
    across /= np.sqrt(across @ across)
    n = across + side * 5e-9 * d / (d @ d)
    n /= np.sqrt(n @ n)
    inward = -p + (p @ n) * n
    inward /= np.sqrt(inward @ inward)
    a = p + 0.02 * inward + side * 1e-12 * n
    R = PC.sphere_radius_of("mie")
    types = np.zeros(1, dtype=CV.PMT_TYPE_DTYPE)
    types[0] = (R, 0, 1, 0, 0)
    pmts = np.zeros(1, dtype=CV.PMT_DTYPE)
    pmts["axis"], pmts["position"], pmts["radius"], pmts["collectionEfficiency"] = n, a, 0.30 * R, 0.9
    pmts["quantumEfficiency"], pmts["angularAcceptance"] = 1, 2
    return ph, (PC.standard_functions(), types, pmts, PC.modules_for(PC.IDENTITY))


def test_a_disc_grazed_from_behind_gives_no_hit():
    ph, configuration = grazing_disc(+1)
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    want, want_counters, details = PC.numpy_pmt_hits(ph, *configuration)
    assert details["found"][0] == 0 and -1e-8 < details["c"][0] <= 0.0         # the disc is found, and it is its back
    assert len(got) == len(want) == 0 and counters == want_counters == counters_of()
    # the same disc turned by 1e-8: found from the front, the record reaches the draw with a probability like any other
    ph, configuration = grazing_disc(-1)
    want, want_counters, details = PC.numpy_pmt_hits(ph, *configuration)
    assert details["found"][0] == 0 and 0.0 < details["c"][0] < 1e-8 and details["drawn"][0] and 0.05 < details["P"][0] < 1.0
    seeds = [s for s in range(40) if len(PC.numpy_pmt_hits(ph, *configuration, seed=s)[0])][:2]
    assert seeds
    for seed in seeds:
        got, counters = PC.make_generator(*configuration, seed=seed).ConvertHost(ph)
        assert len(got) == 1 and got.tobytes() == PC.numpy_pmt_hits(ph, *configuration, seed=seed)[0].tobytes() and counters == counters_of()


def test_capacity_smaller_than_the_result_counts_on():
    ph, configuration, full = reference("mie", "identity")[:3]
    gen = PC.make_generator(*configuration)
    out = np.zeros(10, dtype=CV.PMT_HIT_DTYPE)
    n = C.c_size_t()
    rc = _lib.load().clsimhip_pmt_convert_host(gen._h, ph.ctypes.data_as(C.c_void_p), len(ph), out.ctypes.data_as(C.c_void_p), 10, C.byref(n), None)
    assert rc == 0 and n.value == len(full) > 10 and out.tobytes() == full[:10].tobytes()


# ---- create-time refusals ----
def base():
    functions, types, pmts, modules = PC.configuration("two_types", PC.sphere_radius_of("mie"))
    return functions, types.copy(), pmts.copy(), modules[:8].copy()


def test_create_refuses_a_rotation_that_changes_lengths():
    functions, types, pmts, modules = base()
    PC.make_generator(functions, types, pmts, modules)                                     # the base is accepted
    for bad in (PC.TILTED * 1.001, PC.IDENTITY + np.array([[0, 2e-3, 0], [0, 0, 0], [0, 0, 0]]), np.full((3, 3), np.nan)):
        m = modules.copy()
        m["rotation"][5] = np.asarray(bad).reshape(9)
        assert "rotation does change vector length" in refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, types, pmts, m))
    m = modules.copy()
    m["rotation"][5] = (PC.TILTED * (1.0 + 1e-7)).reshape(9)                              # within the reference's 1e-6
    PC.make_generator(functions, types, pmts, m)


def test_create_refuses_a_pmt_axis_that_is_not_a_unit_vector():
    functions, types, pmts, modules = base()
    pmts["axis"][7] *= 1.00001
    assert "not a unit vector" in refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, types, pmts, modules))


def test_create_refuses_a_pmt_outside_its_sphere():
    functions, types, pmts, modules = base()
    pmts["position"][33] = pmts["axis"][33] * (PC.sphere_radius_of("mie") + 1e-6)
    assert "sphere radius too small" in refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, types, pmts, modules))
    pmts["position"][33] = pmts["axis"][33] * (PC.sphere_radius_of("mie") - 1e-6)
    PC.make_generator(functions, types, pmts, modules)


def test_create_refuses_a_module_without_a_type_and_duplicates():
    functions, types, pmts, modules = base()
    for bad in (2, -1):
        m = modules.copy()
        m["type"][3] = bad
        assert "No type information" in refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, types, pmts, m))
    m = np.concatenate([modules, modules[2:3]])
    assert "given twice" in refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, types, pmts, m))
    m = modules.copy()
    m["stringID"][0] = 40000
    assert "does not fit" in refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, types, pmts, m))


def test_create_refuses_what_exceeds_the_limits():
    functions, types, pmts, modules = base()
    R = PC.sphere_radius_of("mie")
    # nine types
    nine = np.repeat(types[:1], 9)
    refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, nine, pmts, modules))
    PC.make_generator(functions, np.repeat(types[:1], 8), pmts, modules)
    # 65 PMTs in a type
    many = np.zeros(65, dtype=CV.PMT_DTYPE)
    many[:] = pmts[0]
    one = types[:1].copy()
    one["numPMTs"] = 65
    refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions, one, many, modules[modules["type"] == 0]))
    one["numPMTs"] = 64
    PC.make_generator(functions, one, many, modules[modules["type"] == 0])
    # 65 functions; 3073 table values; a function with its own abscissae
    refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions + [PC.constant(1.0)] * 61, types, pmts, modules))
    PC.make_generator(functions + [PC.constant(1.0)] * 60, types, pmts, modules)
    held = sum(len(f[3]) for f in functions)
    refused(_lib.ERR_CONFIG, lambda: PC.make_generator(functions + [PC.table(0.0, 1.0, np.zeros(3073 - held))], types, pmts, modules))
    PC.make_generator(functions + [PC.table(0.0, 1.0, np.zeros(3072 - held))], types, pmts, modules)
    start, step, values = M.acceptance_table()
    uneven = CV.I3CLSimFunctionFromTable(start + step * np.arange(len(values)), values)
    refused(_lib.ERR_CONFIG, lambda: CV.PMTHitGenerator([uneven] + [PC.function_object(f) for f in functions[1:]], types, pmts, modules))
    # indices that name nothing are arguments out of range
    bad = pmts.copy()
    bad["quantumEfficiency"][0] = 4
    refused(_lib.ERR_ARGUMENT, lambda: PC.make_generator(functions, types, bad, modules))
    bad = types.copy()
    bad["firstPMT"][1] = 32
    refused(_lib.ERR_ARGUMENT, lambda: PC.make_generator(functions, bad, pmts, modules))
    assert R > 0


# ---- behind a converter: Compile() ----
def test_compile_refusals():
    PC.check_compile_refusals()


# ---- the record ----
def test_records_match_the_header(tmp_path):
    """24-byte hits; every field of the four structs sits where the numpy dtypes put it (include/clsimhip.h compiled as C99)"""
    assert CV.PMT_HIT_DTYPE.itemsize == 24 and CV.PMT_DTYPE.itemsize == 72 and CV.PMT_MODULE_DTYPE.itemsize == 88 and CV.PMT_TYPE_DTYPE.itemsize == 24
    fields = {"clsimhip_pmt_hit": (CV.PMT_HIT_DTYPE, ["identifier", "string_id", "om_id", "pmt", "reserved", "time"]),
              "clsimhip_pmt": (CV.PMT_DTYPE, ["axis", "position", "radius", "collection_efficiency", "quantum_efficiency", "angular_acceptance"]),
              "clsimhip_pmt_module": (CV.PMT_MODULE_DTYPE, ["string_id", "om_id", "type", "reserved", "rotation"]),
              "clsimhip_pmt_type": (CV.PMT_TYPE_DTYPE, ["sphere_radius", "first_pmt", "n_pmts", "glass_gel_survival", "reserved"])}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "clsimhip.h"', "int main(void) {"]
    for name, (_, members) in fields.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (name, member) for member in members]
        lines.append('printf("\\n");')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(out) == 4
    for line in out:
        words = line.split()
        dtype, members = fields[words[0]]
        assert [int(x) for x in words[1:]] == [dtype.itemsize] + [dtype.fields[k][1] for k in dtype.names], line
        assert len(dtype.names) == len(members)
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert re.search(r"sizeof\(clsimhip_pmt_hit\) == 24 \? 1 : -1", header)


# ---- the stand-alone host program under the sanitizers ----
def write_input(path, ph, functions, types, pmts, modules, seed):
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", len(functions), len(types), len(pmts), len(modules), len(ph), seed, 0, 0))
        for fn in functions:
            if fn[0] == "table":
                f.write(struct.pack("<2q3d", 0, len(fn[3]), fn[1], fn[2], 0.0))
                f.write(np.asarray(fn[3], dtype="<f8").tobytes())
            else:
                f.write(struct.pack("<2q3d", 1, 0, 0.0, 0.0, fn[1]))
        for array in (types, pmts, modules, ph):
            f.write(np.ascontiguousarray(array).tobytes())


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/pmt_host_main.cpp and clsim_amd/csrc/pmt_hits.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("pmt_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c", os.path.join(ROOT, "clsim_amd", "csrc", "pmt_hits.cpp"),
                                                                         os.path.join(ROOT, "tests", "pmt_host_main.cpp")], cwd=str(d))
    exe = str(d / "pmt_host_main")
    # (linked without the HIP runtime: the program defines the entry points the generator names)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "pmt_hits.o", "pmt_host_main.o", "-o", exe], cwd=str(d))
    return exe


def run_host_program(exe, tmp_path, ph, configuration, seed=PC.SEED):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(src, ph, *configuration, seed)
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    return run, (np.fromfile(dst, dtype=CV.PMT_HIT_DTYPE) if run.returncode == 0 else None)


def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path):
    ph, configuration = doctored()
    want, counters = PC.make_generator(*configuration).ConvertHost(ph)
    run, hits = run_host_program(host_program, tmp_path, ph, configuration)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    assert run.stdout.split() == ["hits", str(len(want)), "counters"] + [str(counters[k]) for k in CV.PMT_CONDITIONS]
    assert hits.tobytes() == want.tobytes() and len(want) > 0
    # a refused configuration is an error message and a status, nothing the sanitizers report
    functions, types, pmts, modules = configuration
    bad = pmts.copy()
    bad["axis"][3] *= 1.01
    run, _ = run_host_program(host_program, tmp_path, ph[:10], (functions, types, bad, modules))
    assert run.returncode == 1 and "not a unit vector" in run.stderr and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
