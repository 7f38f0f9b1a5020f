"""Round 10 on the GPU: the layer-crossing loop of the run-time compiled pooled kernel (prop_device.hip.h under KPARAMS_BAKED: signed
running sums, the record's address as the only induction variable, the crossed layer's record in one read where it is aligned, index
clamps in two instructions) against the precompiled pooled kernel, which keeps the loop as it was, and the oracle.

The bar is the project's usual one (tests/test_baked_mainline_gpu.py): two bunches of 1 024 steps on continuing RNG streams; sorted
80-byte records, RNG words and hit count equal bit for bit -- pooled baked ("baked_kernel" = 2, clsimhip_baked_info says "baked") =
pooled precompiled ("baked_kernel" = 0) = oracle.  Recipes (tests/walk_loop.py): SPICE-Mie with its tilt, FAST and generic; constant
lengths + tilt; tabulated lengths + tilt (records in global memory); SPICE-Mie without tilt (the carried layer index); SPICE-Mie with
tabulated refractive indices (layer records on no multiple of four words: the three-word read).

The first 256 steps of a bunch are placed by hand: straight down in layer 0 and straight up in the last layer (the last layer on
entry), one and two layers from either end heading for it (the last layer in mid-walk), polar angles next to pi / 2 (dz of both signs
as close to zero as an angle gets, +-5e-6 below kEpsilon, +-2e-5 above), length-0 steps exactly on layer boundaries (round 9's
placement) in both directions, a millimetre in front of the dustiest layers (the absorption budget ends inside the first crossed
layer), and the rest within 1e-3 of +-z in front of the clearest stretches of ice, so that walks are long.

Guard, from the oracle alone and asserted before the GPU is touched (tests/walk_loop.py: guard; tests/test_walk_loop.py runs it on the
CPU as well): per bunch at least 200 photon trips cross >= 5 layers, at least 50 walks end in layer 0 or in the last layer, at least 50
photons are detected, and every placement does what it is there for."""
import numpy as np
import pytest

from tests import common
from tests import walk_loop as W

pytestmark = pytest.mark.gpu


def product_run(name, generic, baked):
    R = W.recipe(name)
    conv = R.make_converter({"kernel": 1, "generic_kernels": generic, "baked_kernel": baked})            # ("kernel" 1: pool)
    n = len(R.steps)
    assert conv.KernelForBunch(n) == "pool"
    lengths, tilt, aniso, flasher, fast = W.RECIPES[name]
    out = []
    for b in range(W.N_BUNCHES):
        conv.EnqueueSteps(R.steps, b)
        ident, ph = conv.GetConversionResult()
        assert ident == b
        info, launched = conv.GetBakedInfo(), conv.GetLastLaunch()
        assert launched == dict(family="pool", lengths=lengths, tilt=tilt, aniso=aniso, flasher=flasher, fast=fast and not generic), (name, b, launched)
        assert info["state"] == ("baked" if baked else "unused") and info["why"] == "", (name, b, info)
        assert not baked or len(info["key"]) == 32, (name, b, info)
        out.append((common.sort_photons(ph).tobytes(), conv.GetRNGState(n).copy(), len(ph)))
    assert conv.GetStatistics()["NumKernelCalls"] == float(W.N_BUNCHES)
    return out


def same(got, want, what):
    assert len(got) == len(want) == W.N_BUNCHES
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], "%s, bunch %d: %d hits, expected %d" % (what, b, g[2], w[2])
        assert g[0] == w[0], "%s, bunch %d: photon records differ" % (what, b)
        assert np.array_equal(g[1], w[1]), "%s, bunch %d: RNG words differ" % (what, b)


@pytest.mark.parametrize("name,generic", W.CASES, ids=["%s-%s" % (n, "generic" if g else "default") for n, g in W.CASES])
def test_walk_loop_matches_the_precompiled_kernel_and_the_oracle(name, generic):
    assert len(W.recipe(name).steps) == W.N_STEPS == 1024
    print("%s: %r" % (name, W.guard(name)))                     # (CPU only: raises before anything is launched)
    oracle = [(o["records"], o["x"], o["count"]) for o in W.oracle_bunches(name)]
    precompiled = product_run(name, generic, 0)
    baked = product_run(name, generic, 2)
    what = "%s (%s)" % (name, "generic" if generic else "default")
    same(precompiled, oracle, what + ", pooled precompiled against the oracle")
    same(baked, oracle, what + ", pooled baked against the oracle")
    same(baked, precompiled, what + ", pooled baked against pooled precompiled")
