"""The two hit makers on records no propagator delivers (tests/hit_records_common.py: edited fixture records, random bits, discs
built around a ray), host side: each host twin against its numpy restatement -- records, order, bits and counters --, the
conditions on those inputs that keep a green test from meaning "everything was dropped", and both stand-alone host programs under
AddressSanitizer and UndefinedBehaviorSanitizer on the same inputs (the out-of-bounds check of the shared definition with
record-derived indices).  No GPU here (tests/test_hit_records_gpu.py has the kernels)."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import converter as CV
from tests import hit_records_common as H
from tests import mcpe_common as M
from tests import pmt_common as PC
from tests.test_pmt_hits import write_input as write_pmt_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
PANCAKES = (H.OVERSIZE, 1.0)                # time_factor 0 and 0.8
ROTATIONS = ("identity", "tilted")


def records_of(name, pancake=H.OVERSIZE):
    return H.set_a(pancake)[0] if name == "A" else H.set_b(pancake)


@functools.lru_cache(maxsize=None)
def mcpe_reference(name, pancake):
    """(records, numpy MCPEs, numpy counters), computed once and left as it is"""
    ph = records_of(name, pancake)
    want, counters, _, _ = H.restated_mcpes(ph, pancake)
    return ph, want, counters


@functools.lru_cache(maxsize=None)
def pmt_reference(name, rotation):
    """(records, configuration, numpy hits, numpy counters, details)"""
    ph = records_of(name)
    configuration = H.pmt_configuration(rotation)
    return (ph, configuration) + H.restated_hits(ph, configuration)


@functools.lru_cache(maxsize=None)
def set_c_reference():
    return [(name, ph, configuration) + H.restated_hits(ph, configuration) for name, ph, configuration in H.set_c()]


# ---- the sets themselves ----
def test_the_sets_are_deterministic_and_hold_what_they_name():
    a, slices = H.set_a()
    assert 7000 < len(a) < 9000 and len(H.set_b()) == 65536
    assert a.tobytes() == H._set_a.__wrapped__(H.OVERSIZE)[0].tobytes()
    assert H.set_b().tobytes() == H._set_b.__wrapped__(H.OVERSIZE, 65536, 20261018).tobytes()
    first = H.first_angle_beyond_int32()
    assert 3.37e9 < first < 3.38e9 and first * H.TWO_O_PI >= 2.0 ** 31 > H.step_ulps(first, -1) * H.TWO_O_PI
    assert H.beyond_int32(a["theta"][slices["theta:int32+"]]).all() and not H.beyond_int32(a["theta"][slices["theta:int32-"]]).any()
    assert np.isnan(a["theta"][slices["theta:snan"]]).all() and (a["theta"][slices["theta:snan"]].view(np.uint32) == 0x7f800001).all()
    assert (a["theta"][slices["theta:negated"]] < 0).all() and (a["phi"][slices["phi:negated"]] < 0).any()
    # the positions rescaled onto the window's edges lie on both sides of each edge, a float or two away
    for pancake in PANCAKES:
        ph, slices = H.set_a(pancake)
        for edge, target in zip(("lo2", "hi2"), H.surface_window(pancake)):
            r2 = np.concatenate([H.r2_of(ph[slices["xyz:%s%+d" % (edge, u)]]) for u in (-2, -1, 0, 1, 2)])
            assert (r2 < target).sum() >= 16 and (r2 > target).sum() >= 16 and np.abs(r2 / target - 1.0).max() < 1e-6
    # every slice is disjoint from the others and the records are told apart by their identifier
    assert sum(s.stop - s.start for s in slices.values()) == len(ph) and len(np.unique(ph["id"])) == len(ph)


# ---- twin against restatement ----
@pytest.mark.parametrize("pancake", PANCAKES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_mcpe_twin_equals_numpy_restatement(name, pancake):
    ph, want, want_counters = mcpe_reference(name, pancake)
    got, counters = H.mcpe_generator(pancake).ConvertHost(ph)
    assert counters == want_counters
    assert len(got) == len(want) > 0
    assert got.tobytes() == want.tobytes()              # same records, same order, same bits
    # a NaN time has one bit pattern, whatever made it
    bits = got["time"].view(np.uint64)
    assert (bits[np.isnan(got["time"])] == H.CANONICAL_NAN).all()


@pytest.mark.parametrize("rotation", ROTATIONS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_pmt_twin_equals_numpy_restatement(name, rotation):
    ph, configuration, want, want_counters, details = pmt_reference(name, rotation)
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    assert counters == want_counters
    assert len(got) == len(want) > 0
    assert got.tobytes() == want.tobytes()


def test_pmt_twin_equals_numpy_restatement_on_set_c():
    for name, ph, configuration, want, want_counters, details in set_c_reference():
        got, counters = PC.make_generator(*configuration).ConvertHost(ph)
        assert counters == want_counters == dict.fromkeys(CV.PMT_CONDITIONS, 0), name
        assert got.tobytes() == want.tobytes(), name


# ---- conditions on the inputs (from the numpy restatement alone) ----
def accepted_mask(ph, out):
    mask = np.zeros(len(ph), dtype=bool)
    mask[np.searchsorted(ph["id"], out["id"])] = True
    assert mask.sum() == len(out)
    return mask


def test_mcpe_inputs_reach_every_code_and_the_deep_branches():
    total = dict.fromkeys(("accepted", "dropped") + CV.MCPE_CONDITIONS, 0)
    nonfinite = beyond = 0
    for pancake in PANCAKES:
        for name in ("A", "B"):
            ph, out, counters = mcpe_reference(name, pancake)
            for k, v in counters.items():
                total[k] += v
            total["accepted"] += len(out)
            total["dropped"] += len(ph) - len(out) - sum(counters.values())
            nonfinite += int((~np.isfinite(out["time"])).sum())
            mask = accepted_mask(ph, out)
            beyond += int((mask & (H.beyond_int32(ph["theta"]) | H.beyond_int32(ph["phi"]))).sum())
    print(total, "non-finite times %d, accepted beyond the int32 quadrant range %d" % (nonfinite, beyond))
    assert all(v >= 16 for v in total.values())          # every McpeCode
    assert nonfinite >= 64 and beyond >= 16
    # each pancake setting on its own, too
    for pancake in PANCAKES:
        ph, out, counters = mcpe_reference("A", pancake)
        assert all(v >= 16 for v in counters.values()) and (~np.isfinite(out["time"])).sum() >= 64
    # pancake = oversize: the time is the photon's unless the correction is 0 x inf or 0 / 0; pancake 1: zero velocities give infinities
    ph, out, _ = mcpe_reference("A", H.OVERSIZE)
    assert np.isnan(out["time"]).sum() >= 16
    ph, out, _ = mcpe_reference("A", 1.0)
    assert np.isinf(out["time"]).sum() >= 16


def test_pmt_inputs_reach_every_code_and_the_deep_branches():
    for rotation in ROTATIONS:
        total = dict.fromkeys(("accepted", "dropped") + CV.PMT_CONDITIONS, 0)
        odd = 0
        for name in ("A", "B"):
            ph, _, out, counters, details = pmt_reference(name, rotation)
            for k, v in counters.items():
                total[k] += v
            total["accepted"] += len(out)
            # (OFF_SURFACE is not a result: a record counted there goes on)
            total["dropped"] += len(ph) - len(out) - counters["unknown_module"] - counters["probability_above_one"]
            odd += int((details["accepted"] & (H.beyond_int32(ph["theta"]) | H.beyond_int32(ph["phi"]))).sum())
        print(rotation, total, "accepted with a NaN or out-of-range angle: %d" % odd)
        assert all(v >= 16 for v in total.values()) and odd >= 16


def test_set_c_takes_the_branches_it_names():
    by_name = {name: (ph, want, details) for name, ph, _, want, _, details in set_c_reference()}
    found = lambda name: by_name[name][2]["found"]
    assert (found("denom_zero") == 0).all() and len(by_name["denom_zero"][1]) == 0           # mu = +inf, c = -0: dropped
    assert (found("denom_below") == 0).all() and (by_name["denom_below"][2]["c"] < 0).all() and len(by_name["denom_below"][1]) == 0
    assert (found("denom_at") == -1).all()                                                      # skipped at the threshold
    ph, want, details = by_name["denom_front"]
    assert (details["found"] == 0).all() and (details["c"] == 1e-8).all() and details["drawn"].all() and 0 < len(want) < len(ph)
    # the NaN-path rule: the later, plain disc replaces the earlier one whose path length is a NaN -- and only in that order
    ph, want, details = by_name["nan_path_first"]
    assert details["double"].all() and (details["found"] == 1).all() and 0 < len(want) < len(ph) and (want["pmt"] == 1).all()
    ph, want, details = by_name["nan_path_second"]
    assert details["double"].all() and (details["found"] == 0).all() and 0 < len(want) < len(ph) and (want["pmt"] == 0).all()
    ph, want, details = by_name["equal_mu"]
    assert details["double"].all() and (details["found"] == 0).all() and 0 < len(want) < len(ph) and (want["pmt"] == 0).all()


# ---- the generators at their limits ----
def test_full_tables_pmt_twin_equals_numpy_restatement():
    ph, configuration = H.full_pmt_case()
    functions, types, pmts, modules = configuration
    assert len(types) == 8 and len(pmts) == 512 and len(functions) == 64 and sum(len(f[3]) for f in functions) == 3072
    want, want_counters, details = H.restated_hits(ph, configuration)
    got, counters = PC.make_generator(*configuration).ConvertHost(ph)
    assert counters == want_counters and got.tobytes() == want.tobytes()
    kind = got["stringID"] % 8
    assert sorted(set(kind)) == list(range(8))                                                  # hits on every type
    assert ((kind == 7) & (got["pmt"] == 63)).any()
    # a record of type 7 with a wavelength beyond the table reached the draw: it read value 3 071
    beyond = (ph["wavelength"] == np.float32(9e-7)) & (ph["stringID"] % 8 == 7)
    assert (details["drawn"] & beyond).any() and len(functions[63][3]) == 48


def test_full_tables_mcpe_twin_equals_numpy_restatement():
    ph, tables, class_of, gen = H.full_mcpe_case()
    assert len(tables) == 8 and sum(len(t[2]) for t in tables) == 4096
    with np.errstate(all="ignore"):
        want, want_counters, P, accepted = M.numpy_mcpes(ph, tables, class_of, M.angular_coefficients(), H.OVERSIZE)
    got, counters = gen.ConvertHost(ph)
    assert counters == want_counters and not any(counters.values()) and got.tobytes() == want.tobytes()
    assert sorted(set(got["stringID"] % 8)) == list(range(8))
    assert ((ph["wavelength"] == np.float32(9e-7)) & (ph["stringID"] % 8 == 7)).any()           # reads value 4 095 (no early exit: no condition is met)


# ---- the stand-alone host programs under the sanitizers ----
def build_host_program(directory, source, main):
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c", os.path.join(ROOT, "clsim_amd", "csrc", source + ".cpp"),
                                                                         os.path.join(ROOT, "tests", main + ".cpp")], cwd=str(directory))
    exe = str(directory / main)
    # (linked without the HIP runtime: the program defines the entry points the generator names)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", source + ".o", main + ".o", "-o", exe],
                          cwd=str(directory))
    return exe


@pytest.fixture(scope="module")
def mcpe_host_program(tmp_path_factory):
    """tests/mcpe_host_main.cpp and clsim_amd/csrc/mcpe.cpp, host code only, with -fsanitize=address,undefined"""
    return build_host_program(tmp_path_factory.mktemp("mcpe_host_main"), "mcpe", "mcpe_host_main")


@pytest.fixture(scope="module")
def pmt_host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("pmt_host_main"), "pmt_hits", "pmt_host_main")


def write_mcpe_input(path, ph, tables, pancake, seed=M.SEED):
    s, d = H.dom_pairs()
    coefficients = M.angular_coefficients()
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", len(tables), len(coefficients), len(s), len(ph), seed, 0, 0, 0))
        f.write(struct.pack("<3d", M.DOM_RADIUS, H.OVERSIZE, pancake))
        for start, step, values in tables:
            f.write(struct.pack("<2q3d", 0, len(values), start, step, 0.0))
            f.write(np.asarray(values, dtype="<f8").tobytes())
        f.write(np.asarray(coefficients, dtype="<f8").tobytes())
        f.write(struct.pack("<4d", -np.inf, np.inf, np.nan, np.nan))                            # I3CLSimFunctionPolynomial's defaults
        for array, dtype in ((s, "<i4"), (d, "<u4"), (s % 2, "<i4"), (ph, ph.dtype)):
            f.write(np.ascontiguousarray(array, dtype=dtype).tobytes())


def run(exe, tmp_path, dtype):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    return done, (np.fromfile(dst, dtype=dtype) if done.returncode == 0 else None)


@pytest.mark.parametrize("pancake", PANCAKES)
def test_mcpe_host_program_runs_clean_under_the_sanitizers(mcpe_host_program, tmp_path, pancake):
    ph = np.concatenate([records_of("A", pancake), records_of("B", pancake)])
    want, counters = H.mcpe_generator(pancake).ConvertHost(ph)
    write_mcpe_input(str(tmp_path / "in.bin"), ph, H.mcpe_tables(), pancake)
    done, mcpes = run(mcpe_host_program, tmp_path, CV.MCPE_DTYPE)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    assert done.stdout.split() == ["mcpes", str(len(want)), "counters"] + [str(counters[k]) for k in CV.MCPE_CONDITIONS]
    assert mcpes.tobytes() == want.tobytes() and len(want) > 0


@pytest.mark.parametrize("rotation", ROTATIONS)
def test_pmt_host_program_runs_clean_under_the_sanitizers(pmt_host_program, tmp_path, rotation):
    cases = [(np.concatenate([records_of("A"), records_of("B")]), H.pmt_configuration(rotation))]
    if rotation == "identity":
        cases += [(ph, configuration) for _, ph, configuration in H.set_c()]
    for ph, configuration in cases:
        want, counters = PC.make_generator(*configuration).ConvertHost(ph)
        write_pmt_input(str(tmp_path / "in.bin"), ph, *configuration, PC.SEED)
        done, hits = run(pmt_host_program, tmp_path, CV.PMT_HIT_DTYPE)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        assert done.stdout.split() == ["hits", str(len(want)), "counters"] + [str(counters[k]) for k in CV.PMT_CONDITIONS]
        assert hits.tobytes() == want.tobytes()
