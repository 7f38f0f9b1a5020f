#!/usr/bin/env python3
"""Static instruction counts of C2's run-time compiled pooled kernel (bench.py's headline configuration: SPICE-Mie with tilt, IC86, DOM
oversize 5), compiled for gfx950 WITHOUT a device through CompileBakedKernel and disassembled (llvm-objdump).
   tools/baked_code_object.py [--asm FILE]      one block of counts; the library is the tree's, or the one CLSIMHIP_LIB names
Two libraries built on one machine are compared by running it once for each (profiles/r09/baked_code_object.txt)."""
import collections, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clsim_amd import _lib
from tests import common
LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "_ZN8clsimhip16prop_pool_kernelILi1ELb1ELb0ELb0ELb1ELb0EEEvNS_7KParamsE"
# the instruction classes round 9 is about
WATCHED = ("v_floor_f32", "v_cvt_i32_f32", "v_cvt_f32_u32", "v_cvt_f32_i32", "v_med3_i32", "v_cndmask_b32", "v_mad_u32_u24", "v_mul_u32_u24",
           "v_lshl_add_u32", "v_add_u32", "v_cmp_eq_f32", "v_cmp_le_f32", "v_cmp_ge_f32", "v_mov_b32", "ds_read_b32", "ds_read2_b32", "ds_read_b64",
           "ds_read_b128")


def main():
    asm_path = sys.argv[sys.argv.index("--asm") + 1] if "--asm" in sys.argv else None
    conv = common.product_converter(common.config("mie"), 1024, pancake=5.0, initialize=False)
    conv.Compile()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c2.co")
        report = conv.CompileBakedKernel(code_path=path)
        assert report["compiled"], report["why"]
        asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + KERNEL, path],
                             check=True, capture_output=True, text=True).stdout
    if asm_path:
        with open(asm_path, "w") as f:
            f.write(asm)
    code = [line.split("//")[0].strip() for line in asm.splitlines() if line.startswith("\t")]
    names = collections.Counter(re.sub(r"_e(32|64)$|_sdwa$|_dpp$", "", line.split()[0]) for line in code)
    print("library          %s" % os.path.relpath(_lib.LIB_PATH, ROOT))
    print("cache key        %s" % report["key"])
    print("instructions     %d" % len(code))
    print("vector (v_*)     %d" % sum(n for k, n in names.items() if k.startswith("v_")))
    print("scalar (s_*)     %d" % sum(n for k, n in names.items() if k.startswith("s_")))
    print("LDS (ds_*)       %d" % sum(n for k, n in names.items() if k.startswith("ds_")))
    print("compares with the +inf literal (0x7f800000): %d" % sum(1 for line in code if line.startswith("v_cmp") and "0x7f800000" in line))
    for k in WATCHED:
        print("  %-16s %d" % (k, names.get(k, 0)))


if __name__ == "__main__":
    main()
