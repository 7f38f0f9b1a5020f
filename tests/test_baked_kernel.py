"""The pooled kernel compiled at run time for one configuration (clsim_amd/csrc/baked_kernel.h), without a GPU: hiprtc compiles for
gfx950 on any host, so what the code object promises can be read here -- the register budget of tests/test_codegen.py, the kernel
argument layout of the precompiled kernel it replaces, and fewer scalar loads than that kernel has (the point of the exercise).
Also: the cache keys, the fallback when the compiler library cannot be loaded, and the source generator under the address and
undefined-behaviour sanitizers as a program of its own."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from clsim_amd import _lib
from tests import common
from tests.test_codegen import LLVM, kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clsim_amd", "csrc")
# bench.py's C2: SPICE-Mie with its tilt, the 86-string detector, DOM oversize factor 5 -- IceCube lengths, tilt, FAST
C2_KERNEL = "_ZN8clsimhip16prop_pool_kernelILi1ELb1ELb0ELb0ELb1ELb0EEEvNS_7KParamsE"


def c2_converter(pancake=5.0):
    conv = common.product_converter(common.config("mie"), 1024, pancake=pancake, initialize=False)
    conv.Compile()
    return conv


@pytest.fixture(scope="module")
def c2(tmp_path_factory):
    """the compiled code object of C2's configuration: path, the compile's report"""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    path = str(tmp_path_factory.mktemp("baked") / "c2.co")
    conv = c2_converter()
    assert list(conv.GetTable("kernel_variant")) == [1.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    report = conv.CompileBakedKernel(code_path=path)
    assert report["compiled"], report["why"]
    print("C2's pooled kernel compiled in %.2f s, key %s" % (report["seconds"], report["key"]))
    return path, report


@pytest.fixture(scope="module")
def precompiled(tmp_path_factory):
    """the library's code object that holds C2's precompiled instantiation"""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    d = tmp_path_factory.mktemp("precompiled")
    lib = shutil.copy(_lib.LIB_PATH, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
    for f in sorted(os.listdir(d)):
        obj = os.path.join(d, f)
        if f.endswith("gfx950") and C2_KERNEL in kernel_metadata(obj):
            return obj
    raise AssertionError("the library does not hold " + C2_KERNEL)


def instructions(obj):
    asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + C2_KERNEL, obj],
                         check=True, capture_output=True, text=True).stdout
    return [line.split("//")[0].strip() for line in asm.splitlines() if line.startswith("\t")]


def kernarg_bytes(obj):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True, text=True).stdout
    for block in notes.split("- .agpr_count:")[1:]:
        if C2_KERNEL in block:
            return int(re.search(r"\.kernarg_segment_size:\s+(\d+)", block).group(1))
    raise AssertionError("no such kernel in " + obj)


def test_the_compile_takes_seconds_not_minutes(c2):
    assert c2[1]["seconds"] < 10.0, c2[1]            # (the bound from which the GPU suite would have to drop keys; measured: 0.6 s)


def test_baked_kernel_keeps_the_register_budget_and_spills_nothing(c2):
    meta = kernel_metadata(c2[0])
    assert list(meta) == [C2_KERNEL], list(meta)          # one instantiation, under the name the launcher asks the module for
    k = meta[C2_KERNEL]
    assert k["vgpr"] <= 80 and k["scratch"] == 0 and k["vgpr_spills"] == 0, k


def test_baked_kernel_has_no_packed_single_precision_arithmetic(c2):
    code = instructions(c2[0])
    assert len(code) > 2000
    packed = re.compile(r"\bv_pk_(mul|add|fma)_f32\b")
    assert not [line for line in code if packed.search(line)]


def test_baked_kernel_takes_the_kernel_arguments_of_the_precompiled_one(c2, precompiled):
    assert kernarg_bytes(c2[0]) == kernarg_bytes(precompiled)


def test_baked_kernel_has_fewer_scalar_loads_than_the_precompiled_one(c2, precompiled):
    def loads(obj):
        return sum(1 for line in instructions(obj) if line.startswith("s_load_dword"))
    baked, shipped = loads(c2[0]), loads(precompiled)
    print("s_load_dword*: %d baked, %d precompiled" % (baked, shipped))
    assert 0 < baked < shipped


def test_cache_keys_follow_the_configuration_and_the_flags(c2):
    flags = "-O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize"
    same_a = c2_converter().CompileBakedKernel(flags=flags)
    same_b = c2_converter().CompileBakedKernel(flags=flags)
    other_value = c2_converter(pancake=4.0).CompileBakedKernel(flags=flags)
    other_flags = c2_converter().CompileBakedKernel(flags=flags + " -DCLSIMHIP_SOMETHING")
    for r in (same_a, same_b, other_value, other_flags):
        assert r["compiled"] and len(r["key"]) == 32, r
    assert same_a["key"] == same_b["key"]
    assert same_b["seconds"] == 0.0                         # (the second one came out of the in-process cache)
    assert len({same_a["key"], other_value["key"], other_flags["key"], c2[1]["key"]}) == 4


CHILD = """
import sys
sys.path.insert(0, %r)
from tests import test_baked_kernel as T
r = T.c2_converter().CompileBakedKernel()
print("COMPILED", int(r["compiled"]))
print("WHY", r["why"])
"""


def test_without_the_compiler_library_the_entry_reports_the_fallback_and_does_not_throw():
    """(the library is looked for once per process: a child process, with CLSIMHIP_HIPRTC_LIBRARY naming no file)"""
    env = dict(os.environ, CLSIMHIP_HIPRTC_LIBRARY="/nonexistent/libhiprtc.so")
    child = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout + child.stderr
    assert "COMPILED 0" in child.stdout and "WHY cannot load hiprtc" in child.stdout, child.stdout


def test_source_generator_and_cache_key_under_the_sanitizers():
    """host code only, as a program with its own main: nothing of it is loaded into this process"""
    subprocess.run(["make", "-s", "-C", CSRC, "baked_source_check"], check=True)
    run = subprocess.run([os.path.join(CSRC, "baked_source_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "baked source check ok" in run.stdout, run.stdout + run.stderr
