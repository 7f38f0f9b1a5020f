"""Cable shadow on the host: the twin (clsimhip_cable_shadow_host) against an independent numpy restatement byte for byte, the
restatement against the same geometric statement in rational arithmetic, properties that need nothing but the arrays, what creation
refuses, and the twin as a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from clsim_amd.synthetic import PHOTON_DTYPE
from tests import cable_shadow_common as S
from tests import hit_records_common as H
from tests import mcpe_common as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def same(twin, want):
    flags, lit, counts = twin
    return flags.tobytes() == want[0].tobytes() and lit.tobytes() == want[1].tobytes() and counts == want[2]


@pytest.mark.parametrize("n_cylinders", [1, 2, 5160])
def test_twin_equals_numpy_on_mixed_records(n_cylinders):
    """fixture records, records aimed at and past the cylinders, and every seventh adversarial one"""
    records, flags, lit, counts = S.reference(n_cylinders)
    shadow = S.make_shadow(S.cylinder_set(n_cylinders))
    assert shadow.num_cylinders == n_cylinders
    assert same(shadow.MakeHost(records), (flags, lit, counts))
    # the comparison shows something: both outcomes, among the aimed records and among the others
    aimed = records["id"] < 6000
    print(n_cylinders, counts, "aimed and shadowed", int(flags[aimed].sum()))
    assert 0.01 * len(records) < counts["shadowed"] < 0.99 * len(records)


@pytest.mark.parametrize("n_cylinders", [1, 2])
def test_twin_equals_numpy_on_the_adversarial_records(n_cylinders):
    """NaNs, infinities, angles beyond the int32 quadrant range, random bits: every bit pattern a record can hold"""
    records, flags, lit, counts = S.reference(n_cylinders, "adversarial")
    assert len(records) > 15000
    assert same(S.make_shadow(S.cylinder_set(n_cylinders)).MakeHost(records), (flags, lit, counts))
    # a NaN in position or angles is never shadowed
    nan = np.zeros(len(records), dtype=bool)
    for k in ("x", "y", "z", "theta", "phi"):
        nan |= np.isnan(records[k])
    assert nan.sum() > 500 and not flags[nan].any()
    # ... nor is an infinite angle, whose sine and cosine are NaNs
    infinite = np.isinf(records["theta"]) | np.isinf(records["phi"])
    assert infinite.sum() > 100 and not flags[infinite].any()
    beyond = H.beyond_int32(records["theta"]) | H.beyond_int32(records["phi"])
    assert beyond.sum() > 500


def test_restatement_equals_exact_geometry():
    """20 000 single-cylinder cases from default_rng(1): the binary64 rule decides as rational arithmetic does on the same binary64
    inputs, but for cases whose exact |q_min| / (r^2 L2) is below 1e-9 (at most 1 % of the cases); at least 0.5 % hit.
    Measured with this family: 334 hits (1.7 %), no disagreement, no case below the margin."""
    P0, d, top, bottom, radius = S.exact_family()
    A, a, L2, r2 = S.cylinder_records(top, bottom, radius)
    n = len(P0)
    got = np.array([S.segment_hits(P0[i:i + 1], d[i:i + 1], A[i:i + 1], a[i:i + 1], L2[i:i + 1], r2[i:i + 1])[0, 0] for i in range(n)])
    hits = left_out = disagreements = 0
    for i in range(n):
        hit, margin = S.exact_case(P0[i], d[i], top[i], bottom[i], radius[i])
        if margin is not None and margin < 1e-9:
            left_out += 1
            continue
        hits += int(hit)
        disagreements += int(hit != got[i])
    print("cases %d, hits %d, disagreements %d, below the margin %d" % (n, hits, disagreements, left_out))
    assert n == 20000 and left_out <= n // 100 and hits >= n // 200
    assert disagreements == 0


def test_lit_records_are_the_unflagged_ones_in_order_and_the_counts_add_up():
    records = S.mixed_records(2)
    flags, lit, counts = S.make_shadow(S.cylinder_set(2)).MakeHost(records)
    assert set(np.unique(flags)) == {0, 1}
    assert lit.tobytes() == records[flags == 0].tobytes()
    assert counts == {"tested": len(records), "shadowed": int(flags.sum())} and counts["tested"] - counts["shadowed"] == len(lit)
    # no record at all
    flags, lit, counts = S.make_shadow(S.cylinder_set(2)).MakeHost(records[:0])
    assert len(flags) == 0 and len(lit) == 0 and counts == {"tested": 0, "shadowed": 0}


def test_permuting_the_cylinders_changes_nothing():
    records = S.mixed_records(5160)
    top, bottom, radius = S.cylinder_set(5160)
    want = S.reference(5160)
    order = np.random.default_rng(9).permutation(len(top))
    assert same(CV.CableShadow(top[order], bottom[order], radius[order], S.DISTANCE).MakeHost(records), want[1:])
    reverse = np.arange(len(top))[::-1]
    assert same(CV.CableShadow(top[reverse], bottom[reverse], radius[reverse], S.DISTANCE).MakeHost(records), want[1:])


def test_distance_zero_is_point_in_cylinder():
    """D = 0: d = 0 for every finite direction, and the record is shadowed iff its position lies in a cylinder -- decided here from
    the position alone, in rational arithmetic, away from the surface"""
    top, bottom, radius = S.cylinder_set(2)
    rng = np.random.default_rng(3)
    n = 4000
    which = rng.integers(0, 2, n)
    u = rng.uniform(-0.1, 1.1, n)[:, None]
    p = (bottom[which] + u * (top[which] - bottom[which]) + rng.standard_normal((n, 3)) * 0.02).astype(np.float32)
    ph = np.repeat(M.fixture_photons("mie")[:1], n)
    ph["x"], ph["y"], ph["z"] = p[:, 0], p[:, 1], p[:, 2]
    ph["theta"], ph["phi"] = rng.uniform(0, np.pi, n), rng.uniform(0, 2 * np.pi, n)
    flags, lit, counts = CV.CableShadow(top, bottom, radius, 0.0).MakeHost(ph)
    assert same((flags, lit, counts), S.restated(ph, (top, bottom, radius), 0.0))
    inside = np.zeros(n, dtype=bool)
    clear = np.ones(n, dtype=bool)
    for i in range(n):
        for c in range(2):
            hit, margin = S.exact_case(p[i].astype(np.float64), np.zeros(3), top[c], bottom[c], radius[c])
            inside[i] |= hit
            clear[i] &= margin is None or margin > 1e-9
    assert 0.1 * n < inside.sum() < 0.9 * n and clear.sum() > 0.99 * n
    assert np.array_equal(flags[clear] == 1, inside[clear])


def refused(top, bottom, radius, distance):
    lib = _lib.load()
    import ctypes as C
    top, bottom, radius = (np.ascontiguousarray(v, dtype=np.float64) for v in (top, bottom, radius))
    h = C.c_void_p()
    code = lib.clsimhip_cable_shadow_create(len(radius), top.ctypes.data_as(C.c_void_p), bottom.ctypes.data_as(C.c_void_p), radius.ctypes.data_as(C.c_void_p),
                                            float(distance), C.byref(h))
    if code == 0:
        lib.clsimhip_cable_shadow_destroy(h)
    return code


def test_creation_refuses_what_the_header_says():
    top, bottom, radius = (np.array(v) for v in S.cylinder_set(3))
    assert refused(top, bottom, radius, 1.0) == 0 and refused(top, bottom, radius, 0.0) == 0
    for bad in (np.nan, np.inf, -np.inf):
        for array in (0, 1, 2):
            args = [top.copy(), bottom.copy(), radius.copy()]
            args[array].reshape(-1)[-1] = bad
            assert refused(*args, 1.0) == _lib.ERR_ARGUMENT, (bad, array)
    for r in (0.0, -0.01, 1e-200, 1e200):           # r <= 0; r^2 zero; r^2 not finite
        args = [top, bottom, radius.copy()]
        args[2][1] = r
        assert refused(*args, 1.0) == _lib.ERR_ARGUMENT, r
    same_ends = top.copy()
    same_ends[2] = bottom[2]                        # L2 = 0
    assert refused(same_ends, bottom, radius, 1.0) == _lib.ERR_ARGUMENT
    long_one = top.copy()
    long_one[0, 2] = 1e200                          # L2 not finite
    assert refused(long_one, bottom, radius, 1.0) == _lib.ERR_ARGUMENT
    for distance in (-1.0, -1e-300, np.nan, np.inf):
        assert refused(top, bottom, radius, distance) == _lib.ERR_ARGUMENT, distance
    assert refused(top[:0], bottom[:0], radius[:0], 1.0) == _lib.ERR_ARGUMENT
    assert b"cylinder" in _lib.load().clsimhip_cable_shadow_last_error(None)
    many = S.MAX_CYLINDERS + 1
    big = S.cylinder_set(S.MAX_CYLINDERS)
    assert refused(*big, 1.0) == 0
    assert refused(np.tile(top, (many, 1))[:many], np.tile(bottom, (many, 1))[:many], np.tile(radius, many)[:many], 1.0) == _lib.ERR_ARGUMENT
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
        CV.CableShadow(top, bottom, -radius, 1.0)
    assert e.value.code == _lib.ERR_ARGUMENT


def test_setter_before_initialize_and_workspace_query():
    from tests import common
    assert CV.CableShadow.WorkspaceBytes(0) > 0
    assert CV.CableShadow.WorkspaceBytes(1 << 20) >= 4 * ((1 << 20) // S.TILE)
    conv = common.product_converter(common.config("c1"), 512, initialize=False)
    shadow = S.make_shadow(S.cylinder_set(2))
    conv.SetCableShadow(shadow)
    conv.SetCableShadow(None)
    conv.SetCableShadow(shadow)
    conv.Compile()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/cable_shadow_host_main.cpp with clsim_amd/csrc/cable_shadow.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("cable_shadow_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    sources = [os.path.join(ROOT, "clsim_amd", "csrc", "cable_shadow.cpp"), os.path.join(ROOT, "tests", "cable_shadow_host_main.cpp")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c"] + sources, cwd=str(d))
    exe = str(d / "cable_shadow_host_main")
    # (linked without the HIP runtime: the program defines the entry points the file names)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "cable_shadow.o", "cable_shadow_host_main.o",
                           "-o", exe], cwd=str(d))
    return exe


def run_program(exe, tmp_path, cylinders, distance, records):
    top, bottom, radius = cylinders
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(radius), len(records)], dtype=np.uint64).tobytes())
        f.write(np.array([distance], dtype=np.float64).tobytes())
        for array in (top, bottom, radius):
            f.write(np.ascontiguousarray(array, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(records, dtype=PHOTON_DTYPE).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    return run, (np.fromfile(dst, dtype=np.uint8) if run.returncode == 0 else None)


@pytest.mark.parametrize("n_cylinders,which", [(2, "adversarial"), (5160, "mixed")])
def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path, n_cylinders, which):
    records, flags, lit, counts = S.reference(n_cylinders, which)
    run, out = run_program(host_program, tmp_path, S.cylinder_set(n_cylinders), S.DISTANCE, records)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout.split() == ["lit", str(len(lit)), "tested", str(counts["tested"]), "shadowed", str(counts["shadowed"])]
    assert out[:len(records)].tobytes() == flags.tobytes() and out[len(records):].tobytes() == lit.tobytes()


def test_host_program_reports_a_short_input(host_program, tmp_path):
    src = tmp_path / "short.bin"
    src.write_bytes(np.array([3, 5], dtype=np.uint64).tobytes())
    run = subprocess.run([host_program, str(src), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "too short" in run.stderr
