"""Event statistics on the host: the twin (clsimhip_event_statistics_host) against the restatement in Python integers byte for byte,
properties that need nothing but the arrays (order, partition), the two helpers, the bridge to the reference's binary64 running sum,
what the C ABI refuses, and the twin as a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import event_statistics_common as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ES = CV.EventStatistics


def test_record_layout():
    assert CV.EVENT_STATISTICS_DTYPE.itemsize == 144
    assert [CV.EVENT_STATISTICS_DTYPE.fields[n][1] for n in CV.EVENT_STATISTICS_DTYPE.names] == [0, 4, 8, 16, 24, 72, 120, 132]


def test_every_exponent_both_signs_and_every_count():
    """254 finite exponents, subnormals, +-0, with num_photons 0, 1 and 2^32 - 1: one record, without a table"""
    steps, photons = E.exponent_case()
    assert len(steps) == 3 * len(photons) and len(photons) == 2 * (3 + 3 * 254)
    got = ES.MakeHost(steps, photons)
    E.same(got, E.restate(steps, photons))
    # record by record too: every term alone
    for k in range(0, len(steps), 37):
        E.same(ES.MakeHost(steps[k:k + 1], photons[k % len(photons):k % len(photons) + 1]), E.restate(steps[k:k + 1], photons[k % len(photons):k % len(photons) + 1]))
    # positive weights only: the largest sums of the set
    keep = steps["weight"].view(np.uint32) >> 31 == 0
    pos = ES.MakeHost(steps[keep], photons[photons["weight"].view(np.uint32) >> 31 == 0])
    E.same(pos, E.restate(steps[keep], photons[photons["weight"].view(np.uint32) >> 31 == 0]))
    assert E.value_of(pos[0]["generatedSum"][0]) > 1 << 300


def test_non_finite_weights_are_counted_not_summed():
    steps, photons = E.exponent_case(with_specials=True)
    got = ES.MakeHost(steps, photons)
    E.same(got, E.restate(steps, photons))
    r = got[0][0]
    # steps: per count 0 / 1 / 2^32 - 1: +inf, -inf and four NaNs; with count 0 all six are NaN terms
    assert r["generatedSpecial"].tolist() == [2, 2, 6 + 4 + 4] and r["atDOMsSpecial"].tolist() == [1, 1, 4]
    assert r["atDOMsCount"] == len(photons) and r["generatedCount"] == int(steps["num"].astype(np.uint64).sum())
    for bits, num, want in ((0x7f800000, 0, [0, 0, 1]), (0x7f800000, 5, [1, 0, 0]), (0xff800000, 5, [0, 1, 0]), (0xffc00000, 5, [0, 0, 1])):
        one = ES.MakeHost(E.make_steps([num], [bits], [0]), None)[0][0]
        assert one["generatedSpecial"].tolist() == want and not one["generatedSum"].any() and one["generatedCount"] == num


@pytest.mark.parametrize("table", ["consecutive", "scattered"])
def test_interleaved_particles_unknown_identifiers_and_masks(table):
    steps, photons, p, masked = E.interleaved_case()[table]
    got = ES.MakeHost(steps, photons, p, masked)
    want = E.restate(steps, photons, p, masked)
    E.same(got, want)
    assert all(v > 0 for v in want[1].values()) and (got[0]["atDOMsCount"] > 0).all() and got[0]["id"].tolist() == p["id"].tolist()
    assert got[0]["frame"].tolist() == p["frame"].tolist()
    # without the mask more photons count; the entries that name no frame change nothing
    E.same(ES.MakeHost(steps, photons, p, masked[:4]), want)
    assert ES.MakeHost(steps, photons, p)[0]["atDOMsCount"].sum() == got[0]["atDOMsCount"].sum() + want[1]["masked"]


def test_no_table_and_an_empty_table():
    steps, photons, p, masked = E.interleaved_case()["scattered"]
    # no table: one record, identifier 0 and frame 0; the mask's frame is 0
    none = ES.MakeHost(steps, photons, None, np.array([(0, 1, 1), (7, 1, 2)], dtype=CV.MCPE_MASK_DTYPE))
    E.same(none, E.restate(steps, photons, None, np.array([(0, 1, 1), (7, 1, 2)], dtype=CV.MCPE_MASK_DTYPE)))
    assert len(none[0]) == 1 and none[0]["id"][0] == 0 and none[0]["frame"][0] == 0 and none[1]["masked"] > 0 and none[1]["unknown_particle"] == 0
    # an empty table: no record, everything unknown
    empty = ES.MakeHost(steps, photons, p[:0], masked)
    E.same(empty, E.restate(steps, photons, p[:0], masked))
    assert len(empty[0]) == 0 and empty[1] == {"unknown_particle": len(photons), "masked": 0, "unknown_step_particle": len(steps)}
    # no records at all
    nothing = ES.MakeHost(None, None, p)
    assert len(nothing[0]) == len(p) and not nothing[0]["generatedSum"].any() and nothing[0]["id"].tolist() == p["id"].tolist()


def test_shuffling_changes_no_byte_and_bunches_add_exactly():
    steps, photons, p, masked = E.interleaved_case()["consecutive"]
    sx, px = E.exponent_case(with_specials=True)
    sx["id"] = p["id"][np.arange(len(sx)) % len(p)]
    px["id"] = p["id"][np.arange(len(px)) % 3]
    steps, photons = np.concatenate([steps, sx]), np.concatenate([photons, px])
    whole = ES.MakeHost(steps, photons, p, masked)
    rng = np.random.default_rng(2)
    E.same(ES.MakeHost(steps[rng.permutation(len(steps))], photons[rng.permutation(len(photons))], p, masked), whole)
    # a bunch split in two (anywhere) and added up
    for cut_s, cut_p in ((0, len(photons)), (len(steps) // 3, len(photons) // 2), (len(steps) - 1, 1)):
        a, ca = ES.MakeHost(steps[:cut_s], photons[:cut_p], p, masked)
        b, cb = ES.MakeHost(steps[cut_s:], photons[cut_p:], p, masked)
        total = np.array([ES.Add(x, y) for x, y in zip(a, b)], dtype=CV.EVENT_STATISTICS_DTYPE)
        assert total.tobytes() == whole[0].tobytes() and {k: ca[k] + cb[k] for k in ca} == whole[1]


def test_add_carries_through_all_words():
    a = np.zeros(1, dtype=CV.EVENT_STATISTICS_DTYPE)[0]
    b = a.copy()
    a["generatedSum"] = [0xFFFFFFFFFFFFFFFF] * 5 + [0]
    a["atDOMsSum"] = E.words_of(-5)
    a["id"], a["frame"] = 9, 4
    b["generatedSum"] = [1, 0, 0, 0, 0, 0]
    b["atDOMsSum"] = E.words_of(3)
    b["id"], b["frame"] = 1, 1
    b["generatedCount"], b["atDOMsCount"], b["generatedSpecial"], b["atDOMsSpecial"] = 7, 8, [1, 2, 3], [4, 5, 6]
    c = ES.Add(a, b)
    assert c["generatedSum"].tolist() == [0, 0, 0, 0, 0, 1] and E.value_of(c["atDOMsSum"]) == -2 and (c["id"], c["frame"]) == (9, 4)
    assert c["generatedCount"] == 7 and c["atDOMsCount"] == 8 and c["generatedSpecial"].tolist() == [1, 2, 3] and c["atDOMsSpecial"].tolist() == [4, 5, 6]
    assert _lib.load().clsimhip_event_statistics_add(None, None) == _lib.ERR_ARGUMENT


def test_weight_rounds_once_to_nearest_even():
    values = [0, 1, -1, (1 << 53) + 1, (1 << 53) + 3, -((1 << 53) + 1), (1 << 54) + 2, (1 << 54) + 6,   # ties: to even, down and up
              (1 << 200) + (1 << 147) + 1, (1 << 200) + (1 << 147), (1 << 200) + (1 << 148) + (1 << 147),      # the 54th bit with and without sticky bits far below
              (1 << 340) - 1, -(1 << 340), (1 << 383) - 1, -(1 << 383), ((1 << 53) - 1) << 97, (1 << 149), 3 << 148, (1 << 54) - 1]
    rng = np.random.default_rng(4)
    for _ in range(300):
        bits = int(rng.integers(1, 383))
        v = int.from_bytes(rng.bytes(48), "little") >> (384 - bits)
        values += [v, -v]
    for v in values:
        got = ES.Weight(E.words_of(v), [0, 0, 0])
        assert E.double_bits(got) == E.double_bits(E.double_of(v)), v
        assert Fraction(got) == Fraction(E.double_of(v))
    assert E.double_bits(ES.Weight(E.words_of(0), [0, 0, 0])) == 0                                    # zero is +0.0
    assert E.double_bits(ES.Weight(E.words_of((1 << 53) + 1), [0, 0, 0])) == E.double_bits(2.0 ** (53 - 149))   # the tie went to even
    assert E.double_bits(ES.Weight(E.words_of((1 << 200) + (1 << 147) + 1), [0, 0, 0])) == E.double_bits(2.0 ** 51 + 2.0 ** -1)     # sticky: up
    for special, want in (([0, 0, 1], 0x7ff8000000000000), ([3, 2, 0], 0x7ff8000000000000), ([1, 0, 0], 0x7ff0000000000000), ([0, 9, 0], 0xfff0000000000000),
                          ([1, 1, 1], 0x7ff8000000000000)):
        assert E.double_bits(ES.Weight(E.words_of(12345), special)) == want


def test_dyadic_weights_are_the_references_running_sum_bit_for_bit():
    """The bridge to the reference: with weights that are multiples of 2^-10 below 2^10 every binary64 partial sum is exact, so the
    reference's own loop -- a sequential binary64 accumulation in the given order, (double)numPhotons * weight per step -- equals the
    delivered double bit for bit."""
    w = E.dyadic_weights()
    num = (np.arange(len(w)) % 900).astype(np.uint32)
    steps, photons = E.make_steps(num, w.view(np.uint32), np.zeros(len(w))), E.make_photons(w.view(np.uint32), np.zeros(len(w)))
    r = ES.MakeHost(steps, photons)[0][0]
    generated, at_doms = np.float64(0.0), np.float64(0.0)
    for n, x in zip(num, w):
        generated += np.float64(n) * np.float64(x)
        at_doms += np.float64(x)
    assert E.double_bits(ES.Weight(r["generatedSum"], r["generatedSpecial"])) == E.double_bits(float(generated))
    assert E.double_bits(ES.Weight(r["atDOMsSum"], r["atDOMsSpecial"])) == E.double_bits(float(at_doms))
    assert generated != 0 and at_doms != 0


def test_the_references_running_sum_stays_within_its_own_error_bound():
    """Arbitrary positive float32 weights, n = 20 000: recursive summation in binary64 has |error| <= gamma_(n-1) * sum|t| with
    gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) -- the bound is the
    reference's own error, nothing measured here."""
    w = E.positive_weights()
    n = len(w)
    r = ES.MakeHost(None, E.make_photons(w.view(np.uint32), np.zeros(n)))[0][0]
    exact = Fraction(E.value_of(r["atDOMsSum"]), 1 << E.UNIT)
    assert exact == sum(Fraction(float(x)) for x in w)                  # the delivered integer IS the exact sum
    running = np.float64(0.0)
    for x in w:
        running += np.float64(x)
    u = Fraction(1, 1 << 53)
    bound = (n - 1) * u * exact / (1 - (n - 1) * u)                       # all terms positive: sum|t| = exact
    assert abs(Fraction(float(running)) - exact) <= bound
    assert abs(Fraction(ES.Weight(r["atDOMsSum"], r["atDOMsSpecial"])) - exact) <= exact * u        # one rounding


def refusal(call):
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        call()
    return e.value.code


def test_the_c_abi_refuses_what_the_header_says():
    lib = _lib.load()
    steps, photons, p, masked = E.interleaved_case()["scattered"]
    out = np.zeros(8, dtype=CV.EVENT_STATISTICS_DTYPE)
    vp = _lib.C.c_void_p
    # null pointers with counts
    assert lib.clsimhip_event_statistics_host(None, 3, None, 0, None, 0, None, 0, vp(out.ctypes.data), None) == _lib.ERR_ARGUMENT
    assert lib.clsimhip_event_statistics_host(None, 0, None, 2, None, 0, None, 0, vp(out.ctypes.data), None) == _lib.ERR_ARGUMENT
    assert lib.clsimhip_event_statistics_host(None, 0, None, 0, None, 0, None, 2, vp(out.ctypes.data), None) == _lib.ERR_ARGUMENT
    assert lib.clsimhip_event_statistics_host(None, 0, None, 0, None, 0, None, 0, None, None) == _lib.ERR_ARGUMENT
    assert lib.clsimhip_event_statistics_host(None, 0, None, 0, None, 0, None, 0, vp(out.ctypes.data), None) == _lib.OK
    # a table that is not strictly increasing
    for bad in (p[[0, 2, 1, 3]], p[[0, 1, 1, 2]]):
        assert refusal(lambda: ES.MakeHost(steps, photons, bad)) == _lib.ERR_ARGUMENT
    # the device call: a short workspace, misaligned and null pointers are refused before anything touches a device
    room = np.zeros(1 << 16, dtype=np.uint8)
    a = (room.ctypes.data + 15) & ~15
    need = ES.WorkspaceBytes(len(p), len(masked))
    assert ES.WorkspaceBytes(0, 0) > 0 and need < (1 << 15) and ES.WorkspaceBytes(1000, 0) - ES.WorkspaceBytes(0, 0) >= 999 * 12 * 4 * 8
    for args in ((a, 4, a, a, 4, a, a, a, need - 1),            # a workspace that is too small
                 (a, 4, a, a, 4, a, a, a + 8, need),            # ... that is not aligned
                 (a + 2, 4, a, a, 4, a, a, a, need),            # steps that are not aligned
                 (a, 4, a + 1, a, 4, a, a, a, need),            # photons
                 (a, 4, a, a, 4, a + 4, a, a, need),            # records
                 (a, 4, a, a + 2, 4, a, a, a, need),            # the counter
                 (a, 4, a, 0, 4, a, a, a, need),                # no counter
                 (0, 4, a, a, 4, a, a, a, need),                # no steps, but four of them
                 (a, 4, a, a, 4, 0, a, a, need),                # no records
                 (a, 4, a, a, 4, a, 0, a, need)):               # no counters
        assert refusal(lambda: ES.MakeDevice(*args, particles=p, masked=masked)) == _lib.ERR_ARGUMENT
    assert not room.any()


def test_setter_before_initialize_and_getter_without_the_stage():
    from tests import common
    conv = common.product_converter(common.config("c1"), 512, initialize=False)
    conv.SetEventStatistics(True)
    conv.SetEventStatistics(False)
    conv.SetEventStatistics(True)
    conv.Compile()
    assert refusal(lambda: conv.GetResultEventStatistics(None)) == _lib.ERR_STATE      # not initialized


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/event_statistics_host_main.cpp with clsim_amd/csrc/event_stats.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("event_statistics_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    sources = [os.path.join(ROOT, "clsim_amd", "csrc", "event_stats.cpp"), os.path.join(ROOT, "tests", "event_statistics_host_main.cpp")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c"] + sources, cwd=str(d))
    exe = str(d / "event_statistics_host_main")
    # (linked without the HIP runtime: the program defines the entry points the file names)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "event_stats.o", "event_statistics_host_main.o",
                           "-o", exe], cwd=str(d))
    return exe


def run_program(exe, tmp_path, steps, photons, particles, masked):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    n_p = 0 if particles is None else len(particles)
    with open(src, "wb") as f:
        f.write(np.array([len(steps), len(photons), n_p, len(masked), particles is not None], dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(steps, dtype=CV.STEP_DTYPE).tobytes())
        f.write(np.ascontiguousarray(photons, dtype=CV.PHOTON_DTYPE).tobytes())
        if n_p:
            f.write(np.ascontiguousarray(particles, dtype=CV.MCPE_PARTICLE_DTYPE).tobytes())
        f.write(np.ascontiguousarray(masked, dtype=CV.MCPE_MASK_DTYPE).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    return run, (np.fromfile(dst, dtype=np.uint8) if run.returncode == 0 else None)


@pytest.mark.parametrize("case", ["scattered", "consecutive", "no_table", "empty_table", "every_exponent"])
def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path, case):
    if case == "every_exponent":
        steps, photons = E.exponent_case(with_specials=True)
        p, masked = None, np.zeros(0, dtype=CV.MCPE_MASK_DTYPE)
    else:
        steps, photons, p, masked = E.interleaved_case()["consecutive" if case == "consecutive" else "scattered"]
        p = None if case == "no_table" else p[:0] if case == "empty_table" else p
    want, counters = E.restate(steps, photons, p, masked)
    run, out = run_program(host_program, tmp_path, steps, photons, p, masked)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout.split() == ["records", str(len(want))]
    n = 144 * len(want)
    assert out[:n].tobytes() == want.tobytes()
    assert out[n:n + 24].view(np.uint64).tolist() == [counters[k] for k in E.COUNTERS]
    total = out[n + 24:n + 168].view(CV.EVENT_STATISTICS_DTYPE)[0]
    assert E.value_of(total["generatedSum"]) == sum(E.value_of(r["generatedSum"]) for r in want)
    assert E.value_of(total["atDOMsSum"]) == sum(E.value_of(r["atDOMsSum"]) for r in want)
    weights = out[n + 168:n + 184].view(np.float64)
    assert E.double_bits(weights[0]) == E.double_bits(E.double_of(E.value_of(total["generatedSum"]), total["generatedSpecial"]))
    assert E.double_bits(weights[1]) == E.double_bits(E.double_of(E.value_of(total["atDOMsSum"]), total["atDOMsSpecial"]))


def test_host_program_reports_a_short_input(host_program, tmp_path):
    src = tmp_path / "short.bin"
    src.write_bytes(np.array([3, 5, 0, 0, 0], dtype=np.uint64).tobytes())
    run = subprocess.run([host_program, str(src), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "too short" in run.stderr
