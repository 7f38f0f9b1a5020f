"""Every propagation kernel instantiation a caller can reach, against the oracle.

The launchers dispatch on (lengths kind, tilt, anisotropy, flasher) -- 24 keys -- and every key exists as a generic and a FAST
instantiation in each of the classic, keep, pooled and pooled-keep families (192 kernels), and as generic / FAST x 4 / 5 axes in
the table maker (12 keys, 48 kernels).  Each has its own register allocation and its own dead code from `if constexpr`; the other
GPU tests launch about forty of them.  Here every (key, mode) of tests/kernel_matrix.py gets one oracle table set and one
converter, and six bunches in a row on continuing RNG streams: classic generic, classic FAST, pooled generic, pooled FAST, and the
pooled generic and pooled FAST kernels compiled at run time for the recipe's configuration, every configuration member of KParams
a literal (clsimhip_set_tuning "kernel", "generic_kernels" and "baked_kernel" between bunches; baked_kernel.h).  The bar is the one of tests/test_parity_gpu.py, unchanged:
the sorted multiset of 80-byte photon records bit-identical, the RNG state words bit-identical, the hit count equal.  After every
bunch clsimhip_get_last_launch must name the instantiation the bunch was meant for: a test that silently ran another kernel fails;
after each of the last two clsimhip_baked_info must say that the run-time compiled kernel ran, under the key the CPU compile
(clsimhip_baked_compile) gives the same configuration.

tests/test_kernel_matrix.py (CPU) is the guard: the recipes compile to their keys, the oracle detects enough with each, and all 96
run-time compiled kernels can be had within the launcher's register budget."""
import numpy as np
import pytest

from oracle import capi
from tests import common
from tests import kernel_matrix as KM
from tests import test_tabulator as TT

pytestmark = pytest.mark.gpu

CASES = [(key, mode) for key in KM.KEYS for mode in KM.MODES]
# (tuning "kernel", tuning "generic_kernels", tuning "baked_kernel") of the six bunches, in this order
BUNCHES = (("classic", 1, 0), ("classic", 0, 0), ("pool", 1, 0), ("pool", 0, 0), ("pool", 1, 2), ("pool", 0, 2))
FAMILY = {("classic", "stop"): "classic", ("classic", "keep"): "keep", ("pool", "stop"): "pool", ("pool", "keep"): "pool_keep"}


@pytest.mark.parametrize("key,mode", CASES, ids=[KM.key_id(k) + "-" + m for k, m in CASES])
def test_four_instantiations_of_a_key_match_the_oracle(key, mode):
    """(Four precompiled instantiations -- and, since the run-time compiled kernel, the two pooled ones once more in that form: six
    bunches.  The name stays, so that the 48 test IDs remain the ones earlier runs recorded.)"""
    cfg = KM.recipe(key, mode)
    steps = cfg["steps"]
    n = len(steps)
    x, a = common.streams(n)
    T = common.oracle_tables(cfg, stop_detected=cfg["stop_detected"])
    conv = common.product_converter(cfg, n, stop_detected=cfg["stop_detected"])
    variant = conv.GetTable("kernel_variant")
    assert list(variant[:5]) == KM.expected_variant(key, mode)
    fast_possible = int(conv.GetTable("fast_variant")[0]) == 1
    # FAST launches are out of reach for the keys KM.NO_FAST_KEYS names, and for no other: nothing else may go without its FAST run
    assert fast_possible == (key not in KM.NO_FAST_KEYS), "fast_variant is %d for %s" % (fast_possible, cfg["name"])
    assert conv.GetLastLaunch() is None
    xo = x
    baked_keys = []
    for bunch, (kernel, generic, baked) in enumerate(BUNCHES):
        conv.SetTuning("kernel", kernel)                    # ("pool": pooled for every bunch size, "pool_min_steps" becomes 0)
        conv.SetTuning("generic_kernels", generic)
        conv.SetTuning("baked_kernel", baked)               # (2: compiled at run time for this configuration, also on a bunch this small)
        assert conv.KernelForBunch(n) == kernel, "%s: a bunch of %d steps would not take the %s kernel" % (cfg["name"], n, kernel)
        ph_o, cnt_o, xo, _ = capi.propagate(T, steps, xo, a, threads=8)
        ph_o = capi.replace_indices_with_ids(ph_o, T.geo)
        conv.EnqueueSteps(steps, bunch)
        ident, ph_p = conv.GetConversionResult()
        what = "%s, bunch %d (%s, %s%s)" % (cfg["name"], bunch, kernel, "generic" if generic else "FAST", ", baked" if baked else "")
        print("%s: %d photons detected" % (what, cnt_o))
        assert ident == bunch and cnt_o >= KM.MIN_HITS, what
        assert len(ph_p) == cnt_o, what
        assert common.sort_photons(ph_o).tobytes() == common.sort_photons(ph_p).tobytes(), what
        assert np.array_equal(conv.GetRNGState(n), xo), what
        want = KM.expected_launch(key, FAMILY[kernel, mode], fast=(not generic) and fast_possible)
        assert conv.GetLastLaunch() == want, (what, conv.GetLastLaunch(), want)
        info = conv.GetBakedInfo()
        if not baked:
            assert info["state"] == "unused", (what, info)            # nothing has asked for the run-time compiled kernel so far
            continue
        # the run-time compiled kernel really ran -- or, for the entries the CPU compile found out of reach, said why it did not
        if (key, mode, "generic" if generic else "fast") in KM.BAKED_OUT_OF_REACH:
            assert info["state"] == "fallback" and info["why"] != "", (what, info)
        else:
            assert info["state"] == "baked" and info["why"] == "", (what, info)
            # (in the process's cache by now: nothing is compiled again)
            assert info["key"] == conv.CompileBakedKernel()["key"], (what, info)
        baked_keys.append(info["key"])
    if fast_possible:
        assert len(set(baked_keys)) == 2, baked_keys
    assert conv.GetStatistics()["NumKernelCalls"] == float(len(BUNCHES)) == 6.0


TAB_CASES = [(key, kind) for key in KM.TAB_KEYS for kind in ("spherical", "spherical5")]


@pytest.mark.parametrize("key,kind", TAB_CASES, ids=[KM.key_id(k) + "-" + kind for k, kind in TAB_CASES])
def test_table_maker_instantiations_match_the_oracle(key, kind):
    """launch_tab_kernel: 12 keys x {4, 5 axes} x {generic, "fast_kernels" = 1}, under the check (and the bars) of
    tests/test_tabulator.py: test_table_matches_the_oracle / test_fast_table_instantiations_match_the_oracle_too -- one oracle run,
    one table maker per instantiation, the reported instantiation asserted after every launch."""
    med_o, med_p = KM.media(key)
    cfg = dict(name=KM.key_id(key), geom=KM.geometry("stop"), med_o=med_o, med_p=med_p, flasher=False, led=None)
    no_fast = {k[:3] for k in KM.NO_FAST_KEYS}
    TT.check_table_against_the_oracle(kind, cfg, 1.0, expect_fast=(0 if key in no_fast else 1), fast_kernels=(False, True), launch_key=key)
