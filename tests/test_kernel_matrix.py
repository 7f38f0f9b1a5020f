"""The guard of tests/test_kernel_matrix_gpu.py, on the CPU: every recipe of tests/kernel_matrix.py is the key it claims to be once
the product has compiled it (a GPU comparison that ran another instantiation than it meant to, or one that compared two empty
photon lists, would prove nothing), and the oracle alone detects enough photons with it."""
import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from oracle import capi
from tests import common
from tests import kernel_matrix as KM

CASES = [(key, mode) for key in KM.KEYS for mode in KM.MODES]


def test_the_matrix_has_every_key_of_the_dispatchers_once():
    assert len(KM.KEYS) == len(set(KM.KEYS)) == 24 and len(KM.TAB_KEYS) == 12 and len(CASES) == 48
    # the launchers' dispatch over lengths x tilt x aniso x flasher, numbered key = 8 * lengths + 4 * tilt + 2 * aniso + flasher (prop_launch.h: dispatch_variant)
    assert sorted(8 * KM.LENGTHS.index(l) + 4 * t + 2 * a + f for l, t, a, f in KM.KEYS) == list(range(24))
    assert KM.LENGTHS == _lib.LENGTHS_KINDS and KM.NO_FAST_KEYS <= set(KM.KEYS)


@pytest.mark.parametrize("key,mode", CASES, ids=[KM.key_id(k) + "-" + m for k, m in CASES])
def test_recipe_compiles_to_its_key_and_the_oracle_detects_enough(key, mode):
    cfg = KM.recipe(key, mode)
    steps = cfg["steps"]
    assert KM.N_STEPS <= len(steps) <= 2048
    # product side: Compile() is host-only; the struct the launchers dispatch on must be the recipe's key
    conv = common.product_converter(cfg, len(steps), initialize=False, stop_detected=cfg["stop_detected"])
    conv.Compile()
    variant = conv.GetTable("kernel_variant")
    assert list(variant[:5]) == KM.expected_variant(key, mode), (variant, key, mode)
    fast = int(conv.GetTable("fast_variant")[0])
    assert fast == int(variant[5])
    print("%s: fast_variant %d" % (cfg["name"], fast))
    # FAST is out of reach for exactly the keys the list names (by construction of their medium), for no other
    assert (fast == 0) == (key in KM.NO_FAST_KEYS), "fast_variant %d for %s" % (fast, cfg["name"])
    assert conv.GetLastLaunch() is None                     # nothing launched yet
    # oracle side, alone
    x, a = common.streams(len(steps))
    T = common.oracle_tables(cfg, stop_detected=cfg["stop_detected"])
    ph, cnt, _, _ = capi.propagate(T, steps, x, a, threads=8)
    print("%s: %d photons detected by the oracle" % (cfg["name"], cnt))
    assert cnt >= KM.MIN_HITS and len(ph) == cnt
    if key[3]:
        source = dict(zip(steps["id"].tolist(), steps["sourceType"].tolist()))
        per_type = np.bincount([source[int(i)] for i in ph["id"]], minlength=2)
        print("%s: %d from Cherenkov steps, %d from flasher steps" % (cfg["name"], per_type[0], per_type[1]))
        assert per_type[0] > 0 and per_type[1] > 0, per_type


def test_launch_report_python_mirror():
    """_lib.launched_dict: the six ints of clsimhip_get_last_launch by name"""
    assert _lib.launched_dict([-1] * 6) is None
    assert _lib.launched_dict([3, 2, 1, 0, 1, 1]) == dict(family="pool_keep", lengths="table", tilt=True, aniso=False, flasher=True, fast=True)
    assert _lib.KERNEL_FAMILIES == ("classic", "keep", "pool", "pool_keep", "tab4", "tab5")
    assert isinstance(CV.I3CLSimStepToPhotonConverterHIP(0).GetLastLaunch(), type(None))
