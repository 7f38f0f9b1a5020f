"""Round 9 on the CPU: the two table words the run-time compiled pooled kernel reads instead of computing, C2's code object without
the instructions they replace, and the guard of tests/test_baked_mainline_gpu.py.

* The fourth word of a tilt distance bin's record (proof bit | byte address of the bin's correction row << 1) and of a layer's record
  (the layer's lower boundary) against restatements in numpy, found IN the LDS image as it is uploaded: SPICE-Mie, synthetic tilt
  tables of 2, 3 and 8 distances (8: the limit of the scalar bins), constant lengths; with tabulated lengths no boundary is stored.
  The proof bit is what an exhaustive numpy restatement of tables.cpp: division_by_reciprocal_is_exact says.
* C2's code object, compiled without a device, has no v_floor_f32 and compares nothing with +inf.
* Every recipe of tests/baked_mainline.py compiles to the instantiation it names, both its run-time compiled kernels can be had, its
  placed steps are where they claim to be (nr ON the edge in the oracle's own arithmetic), and the oracle detects enough."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from oracle import builders as B
from oracle import capi
from tests import baked_mainline as BM
from tests import kernel_matrix as KM
from tests.test_baked_kernel import C2_KERNEL, c2_converter
from tests.test_codegen import LLVM
from tests.test_kernel_matrix import baked_compile_checked


def bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def compiled(name):
    conv = BM.compiled(name)
    return conv, conv.GetTable("lds_image").astype(np.uint32)


def fma32(x, y, z):
    """RN_single(x * y + z) for float32 arrays, through double: the product is exact there, the sum's error is recovered (TwoSum), and
    a sum that lands exactly between two singles is moved off the tie by that error before the one rounding that counts"""
    p = x.astype(np.float64) * y.astype(np.float64)
    z = z.astype(np.float64)
    s = p + z
    t = s - p
    e = (p - (s - t)) + (z - t)
    tie = np.flatnonzero(((s.view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)) & (e != 0))
    s[tie] = np.nextafter(s[tie], np.where(e[tie] > 0, np.inf, -np.inf))
    return s.astype(np.float32)


def division_by_reciprocal_is_exact(b):
    """tables.cpp, restated: a / b == fma(fma(-b, a r, a), r, a r) with r = RN(1 / b) for every significand of a"""
    b = np.float32(b)
    if not (b > np.float32(1e-18) and b < np.float32(1e18)):
        return False
    r = np.float32(1.0) / b
    for start in range(0, 1 << 23, 1 << 21):
        a = (np.arange(start, start + (1 << 21), dtype=np.uint32) | np.uint32(0x3f800000)).view(np.float32)
        q = a * r
        rem = fma32(np.full_like(a, -b), q, a)
        if np.any(fma32(rem, np.full_like(a, r), q) != a / b):
            return False
    return True


def test_fma_restatement_rounds_once():
    # (1 + 2^-23) * (2^-24 - 2^-47) = 2^-24 (1 - 2^-46); added to z = 1 + 2^-23 the exact sum is 2^-70 BELOW the tie between z and
    # 1 + 2^-22.  Rounded to double first it falls on the tie, and then to the even neighbour, 1 + 2^-22: the wrong one.
    x, y, z = np.float32([1.0 + 2.0 ** -23]), np.float32([2.0 ** -24 - 2.0 ** -47]), np.float32([1.0 + 2.0 ** -23])
    assert float(x[0]) * float(y[0]) == 2.0 ** -24 * (1.0 - 2.0 ** -46) and float(y[0]) == 2.0 ** -24 - 2.0 ** -47
    assert (float(x[0]) * float(y[0]) + float(z[0])) == 1.0 + 2.0 ** -23 + 2.0 ** -24           # (what double makes of it: the tie)
    assert fma32(x, y, z)[0] == np.float32(1.0 + 2.0 ** -23)
    assert fma32(-x, y, -z)[0] == np.float32(-(1.0 + 2.0 ** -23))
    assert fma32(np.float32([3.0]), np.float32([5.0]), np.float32([0.25]))[0] == np.float32(15.25)
    assert division_by_reciprocal_is_exact(128.0) and not division_by_reciprocal_is_exact(1e-20)


@pytest.mark.parametrize("name", ["mie", "tilt_nd2", "tilt_nd3", "tilt_nd8", "constant_tilt", "table_tilt"])
def test_tilt_bin_records_carry_the_proof_bit_and_the_row_address(name):
    conv, image = compiled(name)
    tilt = BM.recipe(name).med_o["tilt"]
    nd, nz = len(tilt["distances"]), len(tilt["zcoords"])
    dist = np.asarray(tilt["distances"], dtype=np.float64).astype(np.float32)
    zcorr = np.asarray(tilt["zcorr"], dtype=np.float64).astype(np.float32).reshape(nd, nz)
    fourth = conv.GetTable("tilt_bin_record_fourth_word")
    assert len(fourth) == nd and fourth[0] == 0.0
    fourth = fourth.astype(np.uint64)
    assert np.all(fourth < 2 ** 32)
    all_proven = True
    for j in range(1, nd):
        w = int(fourth[j])
        width = np.float32(dist[j] - dist[j - 1])
        # the proof bit: what it was before the word carried anything else (the exhaustive restatement for SPICE-Mie's widths and
        # the synthetic tables' one width; for the other media the FAST flag below vouches for the bits)
        if name in ("mie", "tilt_nd3"):
            assert (w & 1) == int(division_by_reciprocal_is_exact(width)), (name, j, w)
        all_proven = all_proven and bool(w & 1)
        if not (w & 1):
            assert w == 0
            continue
        row_bytes = w >> 1
        assert row_bytes % 4 == 0 and row_bytes // 4 + 2 * nz <= len(image)
        row = row_bytes // 4
        # the row the kernel interpolates from for bin j is (j - 1, :), the one above it (j, :) follows nz words later
        assert np.array_equal(image[row:row + nz], bits(zcorr[j - 1])), (name, j)
        assert np.array_equal(image[row + nz:row + 2 * nz], bits(zcorr[j])), (name, j)
    # the record itself, in the image: {dist[j], width, 1 / width, fourth word}
    rec = [int(p) for p in np.flatnonzero(image == bits([dist[1]])[0]) if p % 4 == 0 and image[p + 3] == fourth[1]
           and image[p + 1] == bits([np.float32(dist[1] - dist[0])])[0]]
    assert len(rec) == 1
    base = rec[0] - 4
    for j in range(1, nd):
        width = np.float32(dist[j] - dist[j - 1])
        want = [bits([dist[j]])[0], bits([width])[0], bits([np.float32(1.0) / width])[0], fourth[j]]
        assert list(image[base + 4 * j:base + 4 * j + 4]) == want, (name, j)
    # FAST takes the address without looking at the bit: it must imply every bin proven (tables.cpp: medium_proofs_complete)
    fast = int(conv.GetTable("fast_variant")[0])
    assert not fast or all_proven
    assert fast == int(BM.RECIPES[name][4]) and all_proven


@pytest.mark.parametrize("name", ["mie", "tilt_nd3", "constant_tilt", "mie_index_tables"])
def test_layer_records_carry_the_lower_boundary(name):
    conv, image = compiled(name)
    med_o = BM.recipe(name).med_o
    n = int(med_o["num_layers"])
    thickness, bottom = np.float32(med_o["layers_height"]), np.float32(med_o["layers_z_start"])
    assert conv.GetTable("MEDIUM_LAYER_THICKNESS")[0] == thickness and conv.GetTable("MEDIUM_LAYER_BOTTOM_POS")[0] == bottom
    # mediumLayerBoundary in single precision: a product, then a sum (numpy rounds each to float32)
    want = (np.arange(n, dtype=np.float32) * thickness).astype(np.float32) + bottom
    assert want.dtype == np.float32
    got = conv.GetTable("layer_record_lower_boundary")
    assert len(got) == n and np.array_equal(bits(got), bits(want))
    # ... and in the image: the records {a, b, b400, lower} / {abs, 0, sca, lower}, found by their third words
    third = bits(np.asarray(med_o["b400"] if name != "constant_tilt" else med_o["sca_const"], dtype=np.float64).astype(np.float32))
    at = [int(p) - 2 for p in np.flatnonzero(image == third[0]) if p - 2 + 4 * n <= len(image) and np.array_equal(image[p:p + 4 * n:4], third)]
    assert len(at) == 1, at
    # the records start on a multiple of four words (one wide read in the run-time compiled kernel) unless tabulated refractive
    # indices of 2 x 31 words precede them: that recipe is there for the kernel's other read
    assert (at[0] % 4 != 0) == (name == "mie_index_tables"), at
    assert np.array_equal(image[at[0] + 3:at[0] + 3 + 4 * n:4], bits(want))
    if name == "constant_tilt":
        assert not np.any(image[at[0] + 1:at[0] + 1 + 4 * n:4])


def test_tabulated_lengths_store_no_boundary():
    conv, _ = compiled("table_tilt")
    assert conv.GetTable("kernel_variant")[0] == float(KM.LENGTHS.index("table"))
    with pytest.raises(Exception, match="no table named"):
        conv.GetTable("layer_record_lower_boundary")


def test_c2_code_object_lost_the_instructions_round_9_removed(tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    path = str(tmp_path / "c2.co")
    report = c2_converter().CompileBakedKernel(code_path=path)
    assert report["compiled"], report["why"]
    asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + C2_KERNEL, path],
                         check=True, capture_output=True, text=True).stdout
    code = [line.split("//")[0].strip() for line in asm.splitlines() if line.startswith("\t")]
    assert len(code) > 2000
    names = collections.Counter(line.split()[0] for line in code)
    print("C2 baked: %d instructions, %d vector, %d LDS" % (len(code), sum(v for k, v in names.items() if k.startswith("v_")),
                                                            sum(v for k, v in names.items() if k.startswith("ds_"))))
    # item 1: the tilt z index was the kernel's only floor
    assert not [line for line in code if line.startswith("v_floor_f32")]
    # item 2: +inf reached the padded compares as a literal or through a scalar register; neither is left.  (v_mov_b32 of +inf into a
    # vector register is the logarithm's and the exponential's result for 0 and overflow: no compare.)
    inf_sgprs = set(re.findall(r"^s_mov_b32 (s\d+), 0x7f800000$", "\n".join(code), flags=re.M))
    assert not inf_sgprs, inf_sgprs
    assert not [line for line in code if line.startswith("v_cmp") and "0x7f800000" in line]
    # items 3 and 4: both records come as one wide read each (two more than the kernel had before; recorded, the count is the compiler's)
    print("ds_read_b128: %d" % sum(v for k, v in names.items() if k.startswith("ds_read_b128")))


def test_placed_steps_are_where_they_claim_to_be():
    for name in BM.RECIPES:
        R = BM.recipe(name)
        med_o = R.med_o
        lnx, lny, dist = BM.tilt_literals(med_o)
        conv = BM.compiled(name)
        assert conv.GetTable("getTiltZShift_lnx")[0] == lnx and conv.GetTable("getTiltZShift_lny")[0] == lny
        assert np.array_equal(bits(conv.GetTable("getTiltZShift_data_distancesFromOriginAlongTilt")), bits(dist))
        positions = BM.placed_positions(med_o)
        what = [p[3] for p in positions]
        for j in range(len(dist)):
            x, y, _, _ = positions[what.index("tilt distance %d" % j)]
            # the oracle's own arithmetic on the step's float32 coordinates
            assert BM.tilt_nr(lnx, lny, np.float32(x), np.float32(y)) == dist[j], (name, j)
        st = R.steps[:len(positions)]
        nr = np.array([BM.tilt_nr(lnx, lny, sx, sy) for sx, sy in zip(st["x"], st["y"])])
        on_edge = sum(int(np.any(nr == d)) for d in dist[1:-1])
        assert on_edge == len(dist) - 2 and np.any(nr < dist[0]) and np.any(nr > dist[-1])
        bottom, height, n = float(med_o["layers_z_start"]), float(med_o["layers_height"]), int(med_o["num_layers"])
        assert np.any(st["z"] < bottom) and np.any(st["z"] > bottom + n * height)
        first_z, dz = B.tilt_spacing(med_o["tilt"]["zcoords"])
        assert np.any(st["z"] < first_z) and np.any(st["z"] > first_z + dz * (len(med_o["tilt"]["zcoords"]) - 1))
        cells, x0, y0, inv = conv.GetTable("STRING_PROXIMITY_GRID")[:4]
        ix, iy = (st["x"] - x0) * inv, (st["y"] - y0) * inv
        assert np.any(ix < 0) and np.any(ix >= cells) and np.any(iy < 0) and np.any(iy >= cells)
        assert np.all(R.steps["length"][:BM.PLACED] == 0.0) and np.all(R.steps["num"][:BM.N_STEPS] > 0)


@pytest.mark.parametrize("name", list(BM.RECIPES))
def test_recipe_compiles_to_its_instantiation_and_the_oracle_detects_enough(name, tmp_path):
    R = BM.recipe(name)
    assert KM.N_STEPS <= len(R.steps) <= 2048
    conv = BM.compiled(name)
    v = conv.GetTable("kernel_variant")
    got = (_lib.LENGTHS_KINDS[int(v[0])], bool(v[1]), bool(v[2]), bool(v[3]), bool(int(conv.GetTable("fast_variant")[0])))
    assert got == BM.RECIPES[name] and v[4] == 0.0, (name, got)
    for generic in sorted({g for n, g in BM.CASES if n == name}):
        baked_compile_checked(conv, generic, str(tmp_path / ("%d.co" % generic)), name, False)
    conv.SetTuning("generic_kernels", 0)
    x, a = R.streams
    for bunch in range(2):
        ph, cnt, x, _ = capi.propagate(R.T, R.steps, x, a, threads=8)
        print("%s, bunch %d: %d photons detected by the oracle" % (name, bunch, cnt))
        assert cnt >= KM.MIN_HITS and len(ph) == cnt
