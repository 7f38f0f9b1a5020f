"""The pooled kernel compiled at run time for one configuration (clsim_amd/csrc/baked_kernel.h) against the precompiled kernel
and the oracle.

Every template instantiation runs in this form in tests/test_kernel_matrix_gpu.py, every value of a configuration switch in
tests/test_baked_switches_gpu.py.  Here: what surrounds the kernel -- the cache of modules (two media of one instantiation in one
process), slices, padding, the fallback without the compiler library, and the launcher's own decision with tuning untouched
("baked_kernel" = 1: where it pays and only there) -- on six keys of tests/kernel_matrix.py: the three lengths kinds, tilt on and off,
anisotropy on and off, a flasher key, one key without STOP_PHOTONS_ON_DETECTION.
Per key one oracle table set, two bunches of 1 024 steps on continuing RNG streams, and two converters with the pooled kernel
forced ("kernel" = pool): "baked_kernel" = 0 (precompiled) and 2 (run-time compiled also on small bunches).  The bar is the one of
tests/test_parity_gpu.py: sorted 80-byte records, RNG state words and hit count equal -- between the two converters and between the
run-time compiled kernel and the oracle.  After every bunch the converter must report that the run-time compiled kernel really ran
("baked_state"): a test that silently fell back fails.

What one key computes (oracle result, precompiled result) is computed once and shared by the tests that need it (RESULTS); the
library keeps the compiled modules per process, so a key compiles once however many converters run it."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import capi
from tests import common
from tests import kernel_matrix as KM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {
    "c2": (("icecube", True, False, False), "stop"),            # IceCube lengths + tilt, FAST: the instantiation bench.py's C2 runs
    "lea-aniso": (("icecube", True, True, False), "stop"),      # SPICE-Lea with its anisotropy
    "constant": (("constant", False, False, False), "stop"),
    "table": (("table", False, False, False), "stop"),
    "flasher": (("icecube", False, False, True), "stop"),
    "keep": (("icecube", True, False, False), "keep"),
}
N_BUNCHES = 2
RESULTS = {}


def converter(cfg, n, baked, **tuning):
    conv = common.product_converter(cfg, n, stop_detected=cfg["stop_detected"])
    conv.SetTuning("kernel", "pool")
    conv.SetTuning("baked_kernel", baked)
    for k, v in tuning.items():
        conv.SetTuning(k, v)
    assert conv.KernelForBunch(n) == "pool"
    return conv


def run(conv, steps, bunches, expect_state):
    """[(sorted records as bytes, RNG words, hit count)] of `bunches` bunches in a row"""
    out = []
    for b in range(bunches):
        conv.EnqueueSteps(steps, b)
        ident, ph = conv.GetConversionResult()
        assert ident == b
        if expect_state is not None:
            info = conv.GetBakedInfo()
            assert info["state"] == expect_state, info
        out.append((common.sort_photons(ph).tobytes(), conv.GetRNGState(len(steps)).copy(), len(ph)))
    return out


def oracle_run(cfg, T, steps, bunches):
    x, a = common.streams(len(steps))
    out = []
    for _ in range(bunches):
        ph, cnt, x, _ = capi.propagate(T, steps, x, a, threads=8)
        ph = capi.replace_indices_with_ids(ph, T.geo)
        out.append((common.sort_photons(ph).tobytes(), x, cnt))
    return out


def same(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], "%s, bunch %d: %d hits, expected %d" % (what, b, g[2], w[2])
        assert g[0] == w[0], "%s, bunch %d: photon records differ" % (what, b)
        assert np.array_equal(g[1], w[1]), "%s, bunch %d: RNG words differ" % (what, b)


def key_results(name):
    """cfg, oracle tables, oracle result and precompiled result of a key: once per module"""
    if name not in RESULTS:
        key, mode = KEYS[name]
        cfg = KM.recipe(key, mode)
        T = common.oracle_tables(cfg, stop_detected=cfg["stop_detected"])
        oracle = oracle_run(cfg, T, cfg["steps"], N_BUNCHES)
        conv = converter(cfg, len(cfg["steps"]), 0)
        precompiled = run(conv, cfg["steps"], N_BUNCHES, None)
        assert conv.GetBakedInfo()["state"] == "unused"
        RESULTS[name] = dict(cfg=cfg, T=T, oracle=oracle, precompiled=precompiled)
    return RESULTS[name]


@pytest.mark.parametrize("name", list(KEYS))
def test_baked_kernel_equals_the_precompiled_kernel_and_the_oracle(name):
    R = key_results(name)
    cfg = R["cfg"]
    assert all(o[2] >= KM.MIN_HITS for o in R["oracle"]), [o[2] for o in R["oracle"]]
    conv = converter(cfg, len(cfg["steps"]), 2)
    baked = run(conv, cfg["steps"], N_BUNCHES, "baked")
    info = conv.GetBakedInfo()
    print("%s: key %s, hits %s" % (cfg["name"], info["key"], [b[2] for b in baked]))
    assert len(info["key"]) == 32 and info["why"] == ""
    key, mode = KEYS[name]
    launched = conv.GetLastLaunch()
    assert launched["family"] == ("pool" if mode == "stop" else "pool_keep") and launched["lengths"] == key[0], launched
    same(baked, R["precompiled"], cfg["name"] + ", baked against precompiled")
    same(baked, R["oracle"], cfg["name"] + ", baked against the oracle")


def test_slices_hand_their_streams_on_in_the_baked_kernel():
    R = key_results("c2")
    cfg = R["cfg"]
    conv = converter(cfg, len(cfg["steps"]), 2, slices=16)
    same(run(conv, cfg["steps"], N_BUNCHES, "baked"), R["oracle"], "16 slices per step")


def test_a_bunch_whose_last_quarter_is_padding():
    R = key_results("c2")
    cfg = R["cfg"]
    steps = cfg["steps"].copy()
    steps["num"][3 * len(steps) // 4:] = 0
    oracle = oracle_run(cfg, R["T"], steps, 1)
    assert oracle[0][2] >= KM.MIN_HITS
    n = len(steps)
    same(run(converter(cfg, n, 2), steps, 1, "baked"), oracle, "padded bunch, baked")
    same(run(converter(cfg, n, 0), steps, 1, None), oracle, "padded bunch, precompiled")


def test_two_media_in_one_process_each_run_their_own_kernel():
    """SPICE-Lea without its anisotropy (the c2 key's recipe) and SPICE-Mie compile to the SAME instantiation -- IceCube lengths, tilt,
    FAST -- with different constants: a converter that took the other one's module would show in its records at once."""
    R = key_results("c2")
    lea = R["cfg"]
    steps = lea["steps"]
    n = len(steps)
    mie = dict(common.config("mie"), stop_detected=True)
    mie_precompiled = run(converter(mie, n, 0), steps, N_BUNCHES, None)
    assert mie_precompiled[0][0] != R["precompiled"][0][0]
    a, b = converter(lea, n, 2), converter(mie, n, 2)
    assert a.GetLastLaunch() is None
    got_a, got_b = [], []
    for bunch in range(N_BUNCHES):              # interleaved: Lea, Mie, Lea, Mie
        for conv, got in ((a, got_a), (b, got_b)):
            conv.EnqueueSteps(steps, bunch)
            ident, ph = conv.GetConversionResult()
            assert ident == bunch and conv.GetBakedInfo()["state"] == "baked"
            got.append((common.sort_photons(ph).tobytes(), conv.GetRNGState(n).copy(), len(ph)))
    assert a.GetLastLaunch() == b.GetLastLaunch()
    assert a.GetBakedInfo()["key"] != b.GetBakedInfo()["key"]
    same(got_a, R["precompiled"], "SPICE-Lea beside SPICE-Mie")
    same(got_b, mie_precompiled, "SPICE-Mie beside SPICE-Lea")


CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
from tests import test_baked_kernel_gpu as G
from tests import kernel_matrix as KM
key, mode = G.KEYS["c2"]
cfg = KM.recipe(key, mode)
conv = G.converter(cfg, len(cfg["steps"]), 2)
for records, words, hits in G.run(conv, cfg["steps"], G.N_BUNCHES, "fallback"):
    print("RESULT", hashlib.sha256(records).hexdigest(), hashlib.sha256(words.tobytes()).hexdigest(), hits)
print("WHY", conv.GetBakedInfo()["why"])
"""


def test_without_the_compiler_library_the_precompiled_kernel_runs_and_says_so():
    """The library is looked for once per process, so the converter without it lives in a child process."""
    R = key_results("c2")
    env = dict(os.environ, CLSIMHIP_HIPRTC_LIBRARY="/nonexistent/libhiprtc.so")
    child = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout + child.stderr
    lines = [l.split() for l in child.stdout.splitlines() if l.startswith("RESULT")]
    want = [[hashlib.sha256(r).hexdigest(), hashlib.sha256(w.tobytes()).hexdigest(), str(h)] for r, w, h in R["precompiled"]]
    assert [l[1:] for l in lines] == want
    assert "cannot load hiprtc" in child.stdout
    assert child.stderr.count("runs precompiled") == 1, child.stderr         # said once, not per launch


# ---- the default decision: "baked_kernel" = 1, "kernel" = auto, nothing set by the caller ----
DEFAULT_STEPS = 524288              # converter.cpp: kPooledKernelMinSteps -- from here on a bunch takes the pooled kernel unasked
DEFAULT_LIVE = 1024                 # steps that carry photons; the rest has num = 0, so the oracle's cost is that of 1 024 steps


@pytest.mark.parametrize("name,n,kernel,state", [
    ("mie", DEFAULT_STEPS, "pool", "baked"),                    # IceCube lengths, tilt, FAST: bench.py's C2 -- the instantiation that gains
    ("lea", DEFAULT_STEPS, "pool", "unused"),                   # anisotropy: pooled, but the precompiled kernel (prop_pool_kernel.hip.h: kBakedPays)
    ("mie", DEFAULT_STEPS - 256, "classic", "unused"),          # one workgroup of steps below the threshold: the classic kernel
], ids=["mie-at-the-threshold", "lea-at-the-threshold", "mie-below-the-threshold"])
def test_untouched_tuning_runs_the_baked_kernel_where_it_pays_and_only_there(name, n, kernel, state):
    """What production does by default, observed: no tuning key is set here.  Records and RNG words equal the oracle's; the words of
    the steps without photons stay what they were."""
    from clsim_amd import converter as CV
    cfg = common.config(name)
    x, a = common.streams(DEFAULT_STEPS)                        # (once per module: common.streams keeps them)
    x, a = x[:n], a[:n]
    steps = np.resize(common.steps_for(cfg, DEFAULT_LIVE, seed=41), n)
    steps["num"][DEFAULT_LIVE:] = 0
    T = common.oracle_tables(cfg)
    ph_o, cnt_o, x_o, _ = capi.propagate(T, steps, x, a, threads=8)
    ph_o = capi.replace_indices_with_ids(ph_o, T.geo)
    assert cnt_o >= KM.MIN_HITS
    bias = CV.GetIceCubeDOMAcceptance()
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias),
                            pancakeFactor=5.0, approximateNumberOfWorkItems=n, streams=(x, a))
    assert conv.GetTuning("kernel") == 0 and conv.GetTuning("baked_kernel") == 1 and conv.GetTuning("generic_kernels") == 0
    assert conv.KernelForBunch(n) == kernel
    conv.EnqueueSteps(steps, 7)
    ident, ph_p = conv.GetConversionResult()
    info, launched = conv.GetBakedInfo(), conv.GetLastLaunch()
    print("%s, %d steps: %s, %s, %d photons detected" % (name, n, launched, info, cnt_o))
    assert ident == 7 and len(ph_p) == cnt_o
    assert launched["family"] == kernel and launched["fast"] is True, launched
    assert info["state"] == state and info["why"] == "", info
    assert (len(info["key"]) == 32) == (state == "baked"), info
    assert common.sort_photons(ph_o).tobytes() == common.sort_photons(ph_p).tobytes()
    x_p = conv.GetRNGState(n)
    assert np.array_equal(x_p, x_o)
    assert np.array_equal(x_p[DEFAULT_LIVE:], x[DEFAULT_LIVE:]) and not np.array_equal(x_p[:DEFAULT_LIVE], x[:DEFAULT_LIVE])
