"""Round 9 on the GPU: the run-time compiled pooled kernel, whose per-trip index arithmetic reads table words where the precompiled
kernel computes (prop_device.hip.h under KPARAMS_BAKED: tilt z index, tilt distance bin, correction row address, layer boundary),
against the precompiled pooled kernel and the oracle.

The bar is the one of tests/test_baked_switches_gpu.py: two bunches on continuing RNG streams; sorted 80-byte records, RNG words and
hit count equal bit for bit -- pooled baked ("baked_kernel" = 2) = pooled precompiled ("baked_kernel" = 0) = oracle.  The recipes are
those of tests/baked_mainline.py: SPICE-Mie with its tilt (FAST and generic), synthetic tilt tables of 2, 3 and 8 distances, constant
lengths + tilt, and tabulated lengths + tilt (the path that keeps its arithmetic), each with steps placed on layer boundaries, beyond
the layers and the tilt table in z, left of, right of and exactly ON the tilt distances, and outside the string proximity map.
tests/test_baked_mainline.py (CPU) is the guard: instantiations, placement, and at least KM.MIN_HITS photons per bunch."""
import numpy as np
import pytest

from oracle import capi
from tests import baked_mainline as BM
from tests import common
from tests import kernel_matrix as KM

pytestmark = pytest.mark.gpu

N_BUNCHES = 2
_oracle = {}


def oracle_run(name):
    """[(sorted records as bytes, RNG words, hit count)]: computed once per recipe, shared by its cases"""
    if name not in _oracle:
        R = BM.recipe(name)
        x, a = R.streams
        out = []
        for _ in range(N_BUNCHES):
            ph, cnt, x, _ = capi.propagate(R.T, R.steps, x, a, threads=8)
            ph = capi.replace_indices_with_ids(ph, R.T.geo)
            out.append((common.sort_photons(ph).tobytes(), x, cnt))
        _oracle[name] = out
    return _oracle[name]


def product_run(name, generic, baked):
    R = BM.recipe(name)
    conv = R.make_converter({"kernel": 1, "generic_kernels": generic, "baked_kernel": baked})            # ("kernel" 1: pool)
    n = len(R.steps)
    assert conv.KernelForBunch(n) == "pool"
    lengths, tilt, aniso, flasher, fast = BM.RECIPES[name]
    out = []
    for b in range(N_BUNCHES):
        conv.EnqueueSteps(R.steps, b)
        ident, ph = conv.GetConversionResult()
        assert ident == b
        info, launched = conv.GetBakedInfo(), conv.GetLastLaunch()
        assert launched == dict(family="pool", lengths=lengths, tilt=tilt, aniso=aniso, flasher=flasher, fast=fast and not generic), (name, b, launched)
        assert info["state"] == ("baked" if baked else "unused") and info["why"] == "", (name, b, info)
        assert not baked or len(info["key"]) == 32, (name, b, info)
        out.append((common.sort_photons(ph).tobytes(), conv.GetRNGState(n).copy(), len(ph)))
    assert conv.GetStatistics()["NumKernelCalls"] == float(N_BUNCHES)
    return out


def same(got, want, what):
    assert len(got) == len(want) == N_BUNCHES
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], "%s, bunch %d: %d hits, expected %d" % (what, b, g[2], w[2])
        assert g[0] == w[0], "%s, bunch %d: photon records differ" % (what, b)
        assert np.array_equal(g[1], w[1]), "%s, bunch %d: RNG words differ" % (what, b)


@pytest.mark.parametrize("name,generic", BM.CASES, ids=["%s-%s" % (n, "generic" if g else "default") for n, g in BM.CASES])
def test_baked_mainline_matches_the_precompiled_kernel_and_the_oracle(name, generic):
    assert KM.N_STEPS <= len(BM.recipe(name).steps) <= 2048
    oracle = oracle_run(name)
    print("%s: %s photons detected" % (name, [o[2] for o in oracle]))
    assert all(o[2] >= KM.MIN_HITS for o in oracle), [o[2] for o in oracle]
    precompiled = product_run(name, generic, 0)
    baked = product_run(name, generic, 2)
    what = "%s (%s)" % (name, "generic" if generic else "default")
    same(precompiled, oracle, what + ", pooled precompiled against the oracle")
    same(baked, oracle, what + ", pooled baked against the oracle")
    same(baked, precompiled, what + ", pooled baked against pooled precompiled")
