"""Every configuration switch of the pooled kernel as a literal, against the oracle.

The pooled kernel compiled at run time (clsim_amd/csrc/baked_kernel.h) is different code for every configuration: the compiler sees
the values of the 119 configuration members of KParams, deletes the branches on scatter_kind, has_pancake, bias_kind, gen_kind[],
phase_kind, group_kind, has_fixed_abs, num_subdet, dom_in_lds, num_layers and the div_ok bits, and folds arithmetic on the
constants.  tests/test_kernel_matrix_gpu.py runs all its template instantiations, but every recipe there has the same switches.
Here one recipe of tests/parity_recipes.py per value a switch can take (PR.SWITCHES says which recipe is there for which): one
oracle run of two bunches on continuing RNG streams, one converter with the pooled kernel forced and precompiled ("kernel" = pool,
"baked_kernel" = 0) and one with the run-time compiled kernel ("baked_kernel" = 2).  The bar is the one of
tests/test_parity_gpu.py: sorted 80-byte records, RNG state words and hit count equal -- either converter against the oracle, and
the two against each other.  After every bunch the converter must name the pooled family and, where asked for, report that the
run-time compiled kernel ran.

tests/test_kernel_matrix.py (CPU) is the guard: every recipe compiles to the instantiation it claims, its run-time compiled kernel
can be had, and the oracle detects at least KM.MIN_HITS photons in each bunch."""
import numpy as np
import pytest

from oracle import capi
from tests import common
from tests import kernel_matrix as KM
from tests import parity_recipes as PR

pytestmark = pytest.mark.gpu

N_BUNCHES = 2
# Recipes whose bunches cannot take the pooled kernel -- KernelForBunch(n) != "pool" although "kernel" = pool, because the table image
# leaves the waves' pools too little LDS (prop_pool_kernel.hip: pool_kernel_fits) -- with the reason; compared with KernelForBunch both
# ways.  At most two: more would be a finding about the pooled kernel's reach, not a list to grow.
POOL_OUT_OF_REACH = {}
assert len(POOL_OUT_OF_REACH) <= 2 and set(POOL_OUT_OF_REACH) <= set(PR.SWITCHES)


def oracle_run(R):
    x, a = R.streams
    out = []
    for _ in range(N_BUNCHES):
        ph, cnt, x, _ = capi.propagate(R.T, R.steps, x, a, threads=8)
        ph = capi.replace_indices_with_ids(ph, R.T.geo)
        out.append((common.sort_photons(ph).tobytes(), x, cnt))
    return out


def product_run(R, baked, pooled):
    """[(sorted records as bytes, RNG words, hit count)] of N_BUNCHES bunches in a row on a converter of its own"""
    conv = R.make_converter({"kernel": 1, "baked_kernel": baked})            # ("kernel" 1: pool)
    n = len(R.steps)
    assert (conv.KernelForBunch(n) == "pool") == pooled, "%s: KernelForBunch(%d) is %s" % (R.name, n, conv.KernelForBunch(n))
    out = []
    for b in range(N_BUNCHES):
        conv.EnqueueSteps(R.steps, b)
        ident, ph = conv.GetConversionResult()
        assert ident == b
        info, launched = conv.GetBakedInfo(), conv.GetLastLaunch()
        if pooled:
            assert launched["family"] in ("pool", "pool_keep"), (R.name, b, launched)
            assert info["state"] == ("baked" if baked else "unused") and info["why"] == "", (R.name, b, info)
            assert not baked or len(info["key"]) == 32, (R.name, b, info)
        else:
            assert launched["family"] == "classic" and info["state"] == "unused", (R.name, b, launched, info)
        lengths, tilt, aniso, flasher, fast = PR.SWITCH_INSTANTIATIONS[R.name]
        assert (launched["lengths"], launched["tilt"], launched["aniso"], launched["flasher"], launched["fast"]) == (lengths, tilt, aniso, flasher, fast), launched
        out.append((common.sort_photons(ph).tobytes(), conv.GetRNGState(n).copy(), len(ph)))
    assert conv.GetStatistics()["NumKernelCalls"] == float(N_BUNCHES)
    return out


def same(got, want, what):
    assert len(got) == len(want) == N_BUNCHES
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], "%s, bunch %d: %d hits, expected %d" % (what, b, g[2], w[2])
        assert g[0] == w[0], "%s, bunch %d: photon records differ" % (what, b)
        assert np.array_equal(g[1], w[1]), "%s, bunch %d: RNG words differ" % (what, b)


@pytest.mark.parametrize("name", list(PR.SWITCHES))
def test_switch_as_a_literal_matches_the_precompiled_kernel_and_the_oracle(name, tmp_path):
    factory, why = PR.SWITCHES[name]
    R = factory(tmp_path)
    R.name = name
    assert KM.N_STEPS <= len(R.steps) <= 2048
    oracle = oracle_run(R)
    print("%s (%s): %s photons detected" % (name, why, [o[2] for o in oracle]))
    assert all(o[2] >= KM.MIN_HITS for o in oracle), [o[2] for o in oracle]
    pooled = name not in POOL_OUT_OF_REACH
    precompiled = product_run(R, 0, pooled)
    baked = product_run(R, 2, pooled)
    same(precompiled, oracle, name + ", pooled precompiled against the oracle")
    same(baked, oracle, name + ", pooled baked against the oracle")
    same(baked, precompiled, name + ", pooled baked against pooled precompiled")
