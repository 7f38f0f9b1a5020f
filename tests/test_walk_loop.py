"""Round 10 on the CPU: the layer-crossing loop of C2's run-time compiled pooled kernel, read in the code object that is compiled
here without a device (CompileBakedKernel, gfx950), and the index clamps of the per-trip mainline in front of it.

The crossing loop is the kernel's backward-branching block that holds exactly two v_rcp_f32 (the two lengths of the layer walked into)
and an LDS read (that layer's record).  In the parent commit's code object, measured with crossing_loop() below on the disassembly
tools/baked_code_object.py --asm writes (profiles/r10/baked_code_object.txt), that block holds

    P = 26 vector instructions (v_*) and 2 LDS reads (ds_read2_b32 + ds_read_b32),

among them four v_mul_f32 by the +-1 select (v_cndmask_b32 v, 1.0, -1.0) and two integer adds (the layer index and the record's
address).  This tree's block holds 21 and one ds_read_b128.  The test asserts what the issue sets:

* no v_mul_f32 of the block has the +-1 select as an operand,
* the block's only integer add is the one that advances the address the LDS read uses,
* at most P - 5 = 21 vector instructions,
* and, in the mainline in front of the loop, no v_med3_i32 is fed by a v_mov_b32 of a literal: the four index clamps there (string
  map x and y, tilt z, layer) are v_cvt_u32_f32 + v_min_u32 with the bound as a literal.

Also the guard of tests/test_walk_loop_gpu.py: every recipe of tests/walk_loop.py compiles to the instantiation it names, its run-time
compiled kernels can be had within the register limit, and the oracle alone says that its placed steps do what they are placed for."""
import os
import re
import subprocess

import pytest

from clsim_amd import _lib
from tests import walk_loop as W
from tests.test_baked_kernel import C2_KERNEL, c2_converter
from tests.test_codegen import LLVM
from tests.test_kernel_matrix import baked_compile_checked

PARENT_LOOP_VECTOR_INSTRUCTIONS = 26            # P: the parent commit's block, see above
MAINLINE_WINDOW = 200                           # instructions in front of the loop: free_flight_bound, tilt_z_shift, the walk's start

INTEGER_ADDS = ("v_add_u32", "v_sub_u32", "v_subrev_u32", "v_add_co_u32", "v_sub_co_u32", "v_addc_co_u32", "v_subb_co_u32", "v_lshl_add_u32",
                "v_add_lshl_u32", "v_add3_u32", "v_mad_u32_u24", "v_mad_i32_i24", "v_mad_u64_u32", "v_add_i32", "v_sub_i32")


def mnemonic(line):
    return re.sub(r"_e(32|64)$", "", line.split()[0])


def operands(line):
    return [t.strip() for t in line.split(None, 1)[1].split(",")] if len(line.split(None, 1)) > 1 else []


def disassemble(path):
    """[(offset from the kernel's start, instruction text)]"""
    asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + C2_KERNEL, path],
                         check=True, capture_output=True, text=True).stdout
    return parse(asm)


def parse(asm):
    out = []
    for line in asm.splitlines():
        if not line.startswith("\t") or "//" not in line:
            continue
        text, comment = line.split("//", 1)
        m = re.match(r"\s*([0-9A-Fa-f]+):", comment)
        assert m, line
        target = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", comment)
        out.append([int(m.group(1), 16), text.strip(), int(target.group(1), 16) if target else None])
    assert len(out) > 2000
    start = out[0][0]
    return [(addr - start, text, target) for addr, text, target in out]


def crossing_loop(code):
    """(index of the block's first instruction, index of its backward branch): the one backward-branching block with exactly two
    v_rcp_f32 and an LDS read"""
    by_offset = {off: i for i, (off, _, _) in enumerate(code)}
    found = []
    for i, (off, text, target) in enumerate(code):
        if not text.startswith("s_cbranch") or target is None or target > off:
            continue
        first = by_offset[target]
        block = [t for _, t, _ in code[first:i + 1]]
        if sum(1 for t in block if t.startswith("v_rcp_f32")) == 2 and any(t.startswith("ds_read") for t in block) \
                and not any(t.startswith("s_cbranch") for t in block[:-1]):
            found.append((first, i))
    assert len(found) == 1, found
    return found[0]


def vector_instructions(block):
    return [t for t in block if t.startswith("v_")]


def literal_fed_medians(window):
    """the v_med3_i32 of `window` one of whose operands was last written by a v_mov_b32 of a literal"""
    bad = []
    last_write = {}
    for t in window:
        ops = operands(t)
        if mnemonic(t) == "v_med3_i32":
            bad += [(t, last_write[r]) for r in ops[1:] if r in last_write and re.match(r"v_mov_b32(_e32)? v\d+, 0x[0-9a-f]+$", last_write[r])]
        if t.startswith("v_") and ops and re.match(r"v\d+$", ops[0]):
            last_write[ops[0]] = t
    return bad


@pytest.fixture(scope="module")
def c2_code(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    path = str(tmp_path_factory.mktemp("walk_loop") / "c2.co")
    report = c2_converter().CompileBakedKernel(code_path=path)
    assert report["compiled"], report["why"]
    return disassemble(path)


def test_crossing_loop_carries_only_the_reference_arithmetic(c2_code):
    first, last = crossing_loop(c2_code)
    block = [t for _, t, _ in c2_code[first:last + 1]]
    vector = vector_instructions(block)
    reads = [t for t in block if t.startswith("ds_read")]
    print("crossing loop: %d instructions, %d vector, LDS reads %s" % (len(block), len(vector), [mnemonic(t) for t in reads]))
    for t in block:
        print("    " + t)
    # the +-1 select is formed in front of the loop: v_cndmask_b32 v, 1.0, -1.0
    signs = {operands(t)[0] for _, t, _ in c2_code[max(0, first - MAINLINE_WINDOW):first] if mnemonic(t) == "v_cndmask_b32" and operands(t)[1:3] == ["1.0", "-1.0"]}
    assert len(signs) == 1, signs
    by_sign = [t for t in block if mnemonic(t) == "v_mul_f32" and signs & set(operands(t)[1:])]
    assert not by_sign, by_sign
    # one integer add, and it advances the address of the record's read
    adds = [t for t in block if mnemonic(t) in INTEGER_ADDS]
    assert len(adds) == 1 and len(reads) == 1, (adds, reads)
    assert operands(adds[0])[0] == operands(reads[0])[1].split()[0], (adds, reads)
    assert mnemonic(reads[0]) == "ds_read_b128"                        # (C2's layer records are aligned: one wide read)
    assert len(vector) <= PARENT_LOOP_VECTOR_INSTRUCTIONS - 5, len(vector)


def test_mainline_clamps_take_their_bound_as_a_literal(c2_code):
    first, _ = crossing_loop(c2_code)
    window = [t for _, t, _ in c2_code[max(0, first - MAINLINE_WINDOW):first]]
    clamps = [t for t in window if re.match(r"v_min_u32(_e32)? v\d+, 0x[0-9a-f]+, v\d+$", t)]
    print("index clamps in the mainline: %s" % clamps)
    # the string map's two indices, the tilt's z index and the layer index are all formed in this window ...
    assert len(clamps) >= 4, clamps
    assert sum(1 for t in window if mnemonic(t) == "v_cvt_u32_f32") >= 4
    # ... and none of them, nor anything else there, is a median whose bound a v_mov_b32 had to fetch
    assert not literal_fed_medians(window)


def test_the_reading_of_the_disassembly_finds_what_the_parent_had():
    """the helpers on a piece of the parent's own code: a median fed by a literal move is seen, a multiplication by the select is seen"""
    window = ["v_cvt_i32_f32_e32 v5, v20", "v_mov_b32_e32 v21, 0", "v_mov_b32_e32 v20, 0xaa", "v_med3_i32 v5, v5, 0, v20"]
    assert [t for t, _ in literal_fed_medians(window)] == ["v_med3_i32 v5, v5, 0, v20"]
    assert not literal_fed_medians(["v_mov_b32_e32 v20, v9", "v_med3_i32 v5, v5, 0, v20"])
    assert operands("v_cndmask_b32_e64 v29, 1.0, -1.0, s[4:5]")[:3] == ["v29", "1.0", "-1.0"] and mnemonic("v_mul_f32_e32 v36, v29, v36") == "v_mul_f32"


@pytest.mark.parametrize("name", list(W.RECIPES))
def test_recipe_compiles_to_its_instantiation_and_its_placed_steps_do_what_they_are_for(name, tmp_path):
    conv = W.compiled(name)
    v = conv.GetTable("kernel_variant")
    got = (_lib.LENGTHS_KINDS[int(v[0])], bool(v[1]), bool(v[2]), bool(v[3]), bool(int(conv.GetTable("fast_variant")[0])))
    assert got == W.RECIPES[name] and v[4] == 0.0, (name, got)
    for generic in sorted({g for n, g in W.CASES if n == name}):
        baked_compile_checked(conv, generic, str(tmp_path / ("%d.co" % generic)), name, False)
    conv.SetTuning("generic_kernels", 0)
    figures = W.guard(name)
    print("%s: %r" % (name, figures))
