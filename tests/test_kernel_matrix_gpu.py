"""Every propagation kernel instantiation a caller can reach, against the oracle.

The launchers dispatch on (lengths kind, tilt, anisotropy, flasher) -- 24 keys -- and every key exists as a generic and a FAST
instantiation in each of the classic, keep, pooled and pooled-keep families (192 kernels), and as generic / FAST x 4 / 5 axes in
the table maker (12 keys, 48 kernels).  Each has its own register allocation and its own dead code from `if constexpr`; the other
GPU tests launch about forty of them.  Here every (key, mode) of tests/kernel_matrix.py gets one oracle table set and one
converter, and four bunches in a row on continuing RNG streams: classic generic, classic FAST, pooled generic, pooled FAST
(clsimhip_set_tuning "kernel" and "generic_kernels" between bunches).  The bar is the one of tests/test_parity_gpu.py, unchanged:
the sorted multiset of 80-byte photon records bit-identical, the RNG state words bit-identical, the hit count equal.  After every
bunch clsimhip_get_last_launch must name the instantiation the bunch was meant for: a test that silently ran another kernel fails.

tests/test_kernel_matrix.py (CPU) is the guard: the recipes compile to their keys and the oracle detects enough with each."""
import numpy as np
import pytest

from oracle import capi
from tests import common
from tests import kernel_matrix as KM
from tests import test_tabulator as TT

pytestmark = pytest.mark.gpu

CASES = [(key, mode) for key in KM.KEYS for mode in KM.MODES]
# (tuning "kernel", tuning "generic_kernels") of the four bunches, in this order
BUNCHES = (("classic", 1), ("classic", 0), ("pool", 1), ("pool", 0))
FAMILY = {("classic", "stop"): "classic", ("classic", "keep"): "keep", ("pool", "stop"): "pool", ("pool", "keep"): "pool_keep"}


@pytest.mark.parametrize("key,mode", CASES, ids=[KM.key_id(k) + "-" + m for k, m in CASES])
def test_four_instantiations_of_a_key_match_the_oracle(key, mode):
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
    for bunch, (kernel, generic) in enumerate(BUNCHES):
        conv.SetTuning("kernel", kernel)                    # ("pool": pooled for every bunch size, "pool_min_steps" becomes 0)
        conv.SetTuning("generic_kernels", generic)
        assert conv.KernelForBunch(n) == kernel, "%s: a bunch of %d steps would not take the %s kernel" % (cfg["name"], n, kernel)
        ph_o, cnt_o, xo, _ = capi.propagate(T, steps, xo, a, threads=8)
        ph_o = capi.replace_indices_with_ids(ph_o, T.geo)
        conv.EnqueueSteps(steps, bunch)
        ident, ph_p = conv.GetConversionResult()
        what = "%s, bunch %d (%s, %s)" % (cfg["name"], bunch, kernel, "generic" if generic else "FAST")
        print("%s: %d photons detected" % (what, cnt_o))
        assert ident == bunch and cnt_o >= KM.MIN_HITS, what
        assert len(ph_p) == cnt_o, what
        assert common.sort_photons(ph_o).tobytes() == common.sort_photons(ph_p).tobytes(), what
        assert np.array_equal(conv.GetRNGState(n), xo), what
        want = KM.expected_launch(key, FAMILY[kernel, mode], fast=(not generic) and fast_possible)
        assert conv.GetLastLaunch() == want, (what, conv.GetLastLaunch(), want)
    assert conv.GetStatistics()["NumKernelCalls"] == float(len(BUNCHES))


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
