"""The guard of tests/test_kernel_matrix_gpu.py, on the CPU: every recipe of tests/kernel_matrix.py is the key it claims to be once
the product has compiled it (a GPU comparison that ran another instantiation than it meant to, or one that compared two empty
photon lists, would prove nothing), and the oracle alone detects enough photons with it."""
import re

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from oracle import capi
from tests import common
from tests import kernel_matrix as KM
from tests import parity_recipes as PR
from tests.test_codegen import kernel_metadata

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


def baked_compile_checked(conv, generic, path, name, keep, out_of_reach=False):
    """CompileBakedKernel() of a compiled converter as its FAST (generic = 0) or generic (1) pooled launch would ask for it, held to
    what the launcher (prop_pool_kernel.hip.h, baked_kernel.cpp: baked_pool_function) demands before it runs such a module.  Returns
    the report; out_of_reach: the entry is listed in KM.BAKED_OUT_OF_REACH, and then it must NOT be a kernel the launcher would run."""
    conv.SetTuning("generic_kernels", generic)
    report = conv.CompileBakedKernel(code_path=path)
    what = "%s, %s" % (name, "generic" if generic else "FAST")
    v = conv.GetTable("kernel_variant")
    fast = bool(int(conv.GetTable("fast_variant")[0])) and not generic
    symbol = KM.baked_kernel_name(int(v[0]), int(v[1]), int(v[2]), int(v[3]), int(fast), int(keep))
    meta = kernel_metadata(path) if report["compiled"] else {}
    k = meta.get(symbol, {})
    print("%s: key %s, %.2f s, %s %s" % (what, report["key"], report["seconds"], symbol, k))
    if out_of_reach:
        assert not (report["compiled"] and k and k["vgpr"] <= KM.BAKED_MAX_VGPRS and k["scratch"] == 0), (what, report, k)
        return report
    assert report["compiled"] is True and report["why"] == "", (what, report)
    assert re.fullmatch(r"[0-9a-f]{32}", report["key"]), (what, report)
    assert list(meta) == [symbol], (what, list(meta), symbol)         # one kernel, under the name the launcher asks the module for
    assert k["vgpr"] <= KM.BAKED_MAX_VGPRS and k["scratch"] == 0 and k["vgpr_spills"] == 0, (what, k)
    assert report["seconds"] < KM.BAKED_MAX_SECONDS, (what, report)
    return report


def test_baked_out_of_reach_names_entries_of_the_matrix_only():
    assert KM.BAKED_OUT_OF_REACH <= {(key, mode, which) for key, mode in CASES for which in ("fast", "generic")}


@pytest.mark.parametrize("key,mode", CASES, ids=[KM.key_id(k) + "-" + m for k, m in CASES])
def test_both_baked_kernels_of_a_case_can_be_had(key, mode, tmp_path):
    """Every run-time compiled kernel tests/test_kernel_matrix_gpu.py asks for, compiled here (hiprtc needs no device): 24 keys x
    {stop, keep} x {FAST, generic} = 96 code objects.  KM.BAKED_OUT_OF_REACH is compared with this compile both ways."""
    cfg = KM.recipe(key, mode)
    conv = common.product_converter(cfg, len(cfg["steps"]), initialize=False, stop_detected=cfg["stop_detected"])
    conv.Compile()
    assert list(conv.GetTable("kernel_variant")[:5]) == KM.expected_variant(key, mode)
    reports = {}
    for generic, which in ((0, "fast"), (1, "generic")):
        reports[which] = baked_compile_checked(conv, generic, str(tmp_path / (which + ".co")), cfg["name"], mode == "keep",
                                               out_of_reach=(key, mode, which) in KM.BAKED_OUT_OF_REACH)
    if key not in KM.NO_FAST_KEYS:                          # (without FAST both launches take the generic instantiation: one kernel)
        assert reports["fast"]["key"] != reports["generic"]["key"], reports


@pytest.mark.parametrize("name", list(PR.SWITCHES))
def test_baked_kernel_of_a_switch_recipe_can_be_had_and_the_oracle_detects_enough(name, tmp_path):
    """The guard of tests/test_baked_switches_gpu.py: the recipe compiles to the instantiation PR.SWITCH_INSTANTIATIONS names, its
    run-time compiled kernel passes what the launcher demands, and the oracle detects enough in both bunches."""
    R = PR.SWITCHES[name][0](tmp_path)
    assert KM.N_STEPS <= len(R.steps) <= 2048
    conv = R.make_converter(initialize=False)
    v = conv.GetTable("kernel_variant")
    got = (_lib.LENGTHS_KINDS[int(v[0])], bool(v[1]), bool(v[2]), bool(v[3]), bool(int(conv.GetTable("fast_variant")[0])))
    assert got == PR.SWITCH_INSTANTIATIONS[name], (name, got)
    assert v[4] == 0.0 and int(v[5]) == int(got[4])
    baked_compile_checked(conv, 0, str(tmp_path / "switch.co"), name, False)
    x, a = R.streams
    for bunch in range(2):
        ph, cnt, x, _ = capi.propagate(R.T, R.steps, x, a, threads=8)
        print("%s, bunch %d: %d photons detected by the oracle" % (name, bunch, cnt))
        assert cnt >= KM.MIN_HITS and len(ph) == cnt


def test_switch_recipes_cover_the_values_they_are_there_for(tmp_path):
    """What of a recipe's switch can be read back from Compile() (clsimhip_get_table): the pancake factor, the division proofs, the
    sub-detectors' cell grids, whether the DOM templates are part of the LDS image."""
    def compiled(name):
        return PR.SWITCHES[name][0](tmp_path).make_converter(initialize=False)
    ic86 = compiled("ic86")
    assert compiled("no_pancake").GetTable("PANCAKE_FACTOR")[0] == 1.0 and ic86.GetTable("PANCAKE_FACTOR")[0] == 5.0
    assert len(compiled("text_file_geometry").GetTable("div_ok_cells")) == 1 and len(ic86.GetTable("div_ok_cells")) == 2
    assert int(ic86.GetTable("div_ok")[0]) & 1 == 1 and int(compiled("range_restricted_divides").GetTable("div_ok")[0]) & 1 == 0
    # the 576-string detector's image is beyond seven workgroups per CU
    assert compiled("detector_of_576_strings").GetTable("lds_bytes_per_workgroup")[0] > 160 * 1024 / 7 > ic86.GetTable("lds_bytes_per_workgroup")[0]
    # dom_in_lds: the regular detector's strings share two templates of 60 DOMs, which join the LDS image (packed x|y and z: two words per
    # DOM); IC86 has a template per string, 5 160 DOMs, more words than its whole image: they stay in global memory
    regular = compiled("mie_regular")
    assert len(set(np.round(regular.GetTable("geoDomPosStringStartIndexInTemplateDomList")))) == 2
    templates = len(regular.GetTable("geoDomPosTemplatePositionsZ_flat"))
    assert templates == 120 and regular.GetTable("lds_image_words")[0] - ic86.GetTable("lds_image_words")[0] == 2 * templates
    assert len(ic86.GetTable("geoDomPosTemplatePositionsZ_flat")) == 5160 > ic86.GetTable("lds_image_words")[0] / 2
    # generic instantiations reached without "generic_kernels"
    assert {n for n, inst in PR.SWITCH_INSTANTIATIONS.items() if not inst[4]} >= {"photonics_mie", "photonics_wham", "group_velocity_from_dispersion"}
