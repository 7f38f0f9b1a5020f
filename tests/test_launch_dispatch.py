"""CPU: the one mapping from a KVariant's run-time switches to kernel template arguments (clsim_amd/csrc/prop_launch.h: dispatch_variant)
and the launchers' shared check_lengths, exercised by a stand-alone host program (tests/launch_dispatch_main.cpp: no device code, HIP's
API header for its types only).  Every propagation launcher dispatches through this function, so a wrong tag here is a wrong kernel
everywhere; tests/test_kernel_matrix_gpu.py checks the same on the device, instantiation by instantiation."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_dispatch") / "launch_dispatch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "launch_dispatch_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return [line.split() for line in out.stdout.splitlines()]


def header(lines):
    first = lines[0]
    assert first[0] == "codes" and first[3] == "lengths"
    ok, invalid = int(first[1]), int(first[2])
    kinds = [int(x) for x in first[4:7]]
    assert ok == 0 and invalid != 0 and kinds == list(range(kinds[0], kinds[0] + 3))       # CONSTANT, ICECUBE, TABLE are consecutive
    return ok, invalid, kinds


def calls(lines, form):
    """{(lengths, tilt, aniso, flasher, fast): (rc, times the functor ran, tags)}"""
    found = {}
    for f in lines:
        if f[0] == form:
            assert f[1] == "in" and f[7] == "rc" and f[9] == "calls" and f[11] == "tags"
            key = tuple(int(x) for x in f[2:7])
            assert key not in found
            found[key] = (int(f[8]), int(f[10]), tuple(int(x) for x in f[12:17]))
    return found


def test_every_key_reaches_the_functor_with_its_own_tags(lines):
    ok, invalid, kinds = header(lines)
    got = calls(lines, "variant")
    for key in itertools.product(kinds, (0, 1), (0, 1), (0, 1), (0, 1)):       # 3 x 2 x 2 x 2 x 2 = 48
        assert got[key] == (ok, 1, key), key
    assert sum(1 for k in got if k[0] in kinds) == 48


def test_a_lengths_kind_out_of_range_is_refused_without_calling_the_functor(lines):
    ok, invalid, kinds = header(lines)
    for form in ("variant", "tab"):
        got = calls(lines, form)
        for lengths in (kinds[0] - 1, kinds[-1] + 1):
            for rest in itertools.product((0, 1), repeat=4):
                assert got[(lengths,) + rest] == (invalid, 0, (-1, -1, -1, -1, -1)), (form, lengths, rest)


def test_the_table_makers_form_always_compiles_flasher_in(lines):
    ok, invalid, kinds = header(lines)
    got = calls(lines, "tab")
    for lengths, tilt, aniso, fast in itertools.product(kinds, (0, 1), (0, 1), (0, 1)):        # 12 keys x fast
        for flasher in (0, 1):          # (whatever the variant says)
            assert got[(lengths, tilt, aniso, flasher, fast)] == (ok, 1, (lengths, tilt, aniso, 1, fast))


def test_check_lengths(lines):
    ok, invalid, kinds = header(lines)
    got = {f[1]: int(f[2]) for f in lines if f[0] == "check_lengths"}
    assert got == {"null_table": invalid, "one_bin": invalid, "table_ok": ok, "no_table_needed": ok, "below": invalid, "above": invalid}


def test_the_tree_holds_one_dispatch_and_no_mode_macro():
    """the structure this header exists for: one mapping, one declaration of the shared passes, no translation-unit mode macros"""
    src = os.path.join(ROOT, "clsim_amd", "csrc")
    text = {name: open(os.path.join(src, name)).read() for name in sorted(os.listdir(src)) if name.endswith((".hip", ".h", ".cpp"))}
    everything = "\n".join(text.values())
    assert not re.search(r"CLSIMHIP_\w*_UNIT\b", everything)         # (a translation unit is an #include and a launcher, not a mode of a shared file)
    assert everything.count("case CLSIMHIP_LENGTHS_CONSTANT:") == 1 and "#define CASES" not in everything
    for name in ("launch_scan_steps", "launch_assemble_hits"):
        assert everything.count("hipError_t %s(" % name) == 2, name         # its declaration (prop_launch.h) and its definition
        assert text["prop_launch.h"].count("hipError_t %s(" % name) == 1 and text["prop_aux_kernels.hip"].count("hipError_t %s(" % name) == 1
