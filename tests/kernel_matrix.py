"""One recipe per key of the launchers' dispatch -- (lengths kind, tilt, anisotropy, flasher): 3 x 2 x 2 x 2 = 24 -- built on both
sides: the oracle's medium dict and the product's medium through clsimhip_medium_describe -> edit -> clsimhip_medium_create.
tests/test_kernel_matrix.py (CPU: the recipes are what they claim, the oracle detects enough) and tests/test_kernel_matrix_gpu.py
(every instantiation against the oracle) share them.

What the recipes are made of:
  * layer grid, refractive index, Mixed(Liu, HG) scattering: SPICE-Lea for the constant and IceCube kinds; the photonics SPICE-Mie
    table (its own layers and tabulated refractive indices) with SPICE-Lea's scattering object for the table kind, as
    tests/test_parity_gpu.py's table_with_tilt_and_aniso.  Mixed scattering everywhere because the FAST instantiations exist for
    it only (tables.cpp: medium_proofs_complete): a recipe with pure HG could never reach half of its kernels.
  * lengths "constant": one I3CLSimFunctionConstant pair PER LAYER on SPICE-Lea's 171-layer grid -- the scattering and absorption
    lengths of that layer at 400 nm.  (A single layer, as in the homogeneous medium "c1", would make the tilt a no-op: the shifted
    height never selects another layer.  clsimhip_medium_create takes one entry per layer, so this is the form chosen.)
  * tilt: SPICE-Lea's ScalarFieldIceTiltZShift; anisotropy: its absorption length scaling + pre / post scattering transforms.
  * flasher: a second wavelength generator (the 405 nm constant) and a bunch of flasher steps next to a DOM in which the first
    quarter are Cherenkov steps (source type 0), as tests/test_parity_gpu.py's flasher_c1.
  * without STOP_PHOTONS_ON_DETECTION ("keep"): the 60-string detector of common.config("<name>_60"), the largest for which the
    reference's search stays inside its bit mask."""
import ctypes as C
import os

import numpy as np

from clsim_amd import _lib
from clsim_amd import converter as CV
from clsim_amd import synthetic as S
from oracle import builders as B
from tests import common

LENGTHS = ("constant", "icecube", "table")
KEYS = [(lengths, tilt, aniso, flasher) for lengths in LENGTHS for tilt in (False, True) for aniso in (False, True) for flasher in (False, True)]
TAB_KEYS = [(lengths, tilt, aniso) for lengths in LENGTHS for tilt in (False, True) for aniso in (False, True)]
MODES = ("stop", "keep")
N_STEPS = 1024                      # steps per bunch (the issue's range is 1 024 ... 2 048)
MIN_HITS = 50                       # the bar of the existing parity tests (tests/test_pool_kernel_gpu.py, test_parity_gpu.py)

# Keys whose medium cannot pass tables.cpp: medium_proofs_complete BY CONSTRUCTION, i.e. whose FAST instantiations no configuration of
# that key can reach: none.  (Filled in by reasoning about the proofs, never from a run: tests/test_kernel_matrix.py compares it with
# what Compile() reports.)
NO_FAST_KEYS = frozenset()

# (key, mode, "fast" | "generic") whose pooled kernel cannot be had compiled at run time with the configuration as literals ("baked_kernel"):
# none.  Filled from the CPU compile of tests/test_kernel_matrix.py only (clsimhip_baked_compile: hiprtc needs no device), never from a GPU
# run, and compared with it both ways; for an entry the GPU tests expect "fallback" with a reason -- and the same records.
BAKED_OUT_OF_REACH = frozenset()
BAKED_MAX_VGPRS = 80                # prop_pool_kernel.hip.h: the launcher runs the precompiled kernel instead of a module above this, or with scratch
BAKED_MAX_SECONDS = 10.0            # the bound of tests/test_baked_kernel.py


def baked_kernel_name(lengths, tilt, aniso, flasher, fast, keep):
    """baked_source.cpp: baked_kernel_name, restated -- the one kernel of a run-time compiled code object"""
    return "_ZN8clsimhip16prop_pool_kernelILi%dELb%dELb%dELb%dELb%dELb%dEEEvNS_7KParamsE" % (lengths, tilt, aniso, flasher, fast, keep)


ANISO_FIELDS = ("has_anisotropy", "aniso_azimuth", "aniso_k1", "aniso_k2", "has_pre_transform", "pre_renormalize", "pre_matrix",
                "has_post_transform", "post_renormalize", "post_matrix")
TILT_FIELDS = ("has_tilt", "tilt_num_distances", "tilt_num_z", "tilt_distances", "tilt_z_coordinates", "tilt_z_corrections", "tilt_azimuth")
SCATTER_FIELDS = ("scatter_kind", "liu_fraction", "mean_cosine")


def key_id(key):
    lengths, tilt, aniso = key[:3]
    return "-".join([lengths] + [n for n, on in (("tilt", tilt), ("aniso", aniso)) if on] + (["flasher"] if len(key) > 3 and key[3] else []))


def _describe(medium):
    d = _lib.MediumDesc()
    assert _lib.load().clsimhip_medium_describe(medium._h, C.byref(d)) == 0
    return d


_lea = {}


def _spice_lea():
    if not _lea:
        directory = os.path.join(common.ICE, "spice_lea")
        _lea["o"] = B.load_ppc_ice(directory)
        _lea["p"] = CV.MakeIceCubeMediumProperties(iceDataDirectory=directory)
    return _lea["o"], _lea["p"]


def constant_lengths(lea_o):
    """(absorption, scattering) length per layer: SPICE-Lea's at 400 nm (MakeIceCubeMediumProperties.py's formulae at x = 400)"""
    sca = 1.0 / np.asarray(lea_o["b400"], dtype=np.float64)
    a = (lea_o["D"] * np.asarray(lea_o["aDust400"]) + lea_o["E"]) * 400.0 ** -lea_o["kappa"] \
        + lea_o["A"] * np.exp(-lea_o["B"] / 400.0) * (1.0 + 0.01 * np.asarray(lea_o["deltaTau"]))
    return np.ascontiguousarray(1.0 / a), np.ascontiguousarray(sca)


def media(key):
    """(med_o, med_p) for a key (the flasher flag does not touch the medium)"""
    lengths, tilt, aniso = key[:3]
    lea_o, lea_p = _spice_lea()
    lea_d = _describe(lea_p)
    keep = [lea_p]
    if lengths == "table":
        path = common.PHOTONICS["photonics_mie"]
        med_o = B.load_photonics_ice(path)
        med_o["scat"] = lea_o["scat"]
        base = CV.MakeIceCubeMediumPropertiesPhotonics(path)
        keep.append(base)
        d = _describe(base)
        for f in SCATTER_FIELDS:
            setattr(d, f, getattr(lea_d, f))
    else:
        med_o = {k: v for k, v in lea_o.items() if k not in ("aniso", "pre", "post", "tilt")}
        d = _describe(lea_p)
        if lengths == "constant":
            abs_len, sca_len = constant_lengths(lea_o)
            for k in ("alpha", "kappa", "A", "B", "D", "E", "aDust400", "deltaTau", "b400"):
                del med_o[k]
            med_o.update(len_mode="constant", abs_const=abs_len, sca_const=sca_len)
            d.lengths_kind = 0
            d.abs_length, d.sca_length = abs_len.ctypes.data_as(_lib.DP), sca_len.ctypes.data_as(_lib.DP)
            keep += [abs_len, sca_len]
    if aniso:
        for k in ("aniso", "pre", "post"):
            med_o[k] = lea_o[k]
    if tilt:
        med_o["tilt"] = lea_o["tilt"]
    for fields, on in ((ANISO_FIELDS, aniso), (TILT_FIELDS, tilt)):
        for f in fields:
            if on:
                setattr(d, f, getattr(lea_d, f))
            elif f.startswith("has_"):
                setattr(d, f, 0)
    if not tilt:
        d.tilt_num_distances = d.tilt_num_z = 0
    h = C.c_void_p()
    assert _lib.load().clsimhip_medium_create(C.byref(d), C.byref(h)) == 0, _lib.load().clsimhip_last_error(None)
    return med_o, CV.I3CLSimMediumProperties(h, keep=tuple(keep))


_geometries = {}


def geometry(mode):
    if mode not in _geometries:
        _geometries[mode] = common.config("mie_60" if mode == "keep" else "mie")["geom"]
    return _geometries[mode]


def recipe(key, mode):
    """A configuration in the form tests/common.py builds: common.oracle_tables(cfg, stop_detected=...) and
    common.product_converter(cfg, ..., stop_detected=...) take it; cfg["steps"] is the bunch, cfg["stop_detected"] the mode."""
    med_o, med_p = media(key)
    geom = geometry(mode)
    flasher = key[3]
    seed = 101 + KEYS.index(key)
    if flasher:
        # next to the DOM closest to the detector's centre (12 m away, as common.steps_for)
        k = int(np.argmin(np.asarray(geom["x"]) ** 2 + np.asarray(geom["y"]) ** 2 + np.asarray(geom["z"]) ** 2))
        steps = S.flasher_steps(N_STEPS, seed=seed, position=(geom["x"][k] + 12.0, geom["y"][k], geom["z"][k]), pad_to=256)
        steps["sourceType"][:N_STEPS // 4] = 0          # Cherenkov steps in the same bunch
        steps["length"][:N_STEPS // 4] = 0.001
        steps["num"][N_STEPS // 4:N_STEPS // 4 + 20] = 0            # and a few empty ones
    else:
        steps = S.cascade_steps(N_STEPS, seed=seed, pad_to=256)
    return dict(name=key_id(key) + "-" + mode, key=key, mode=mode, geom=geom, med_o=med_o, med_p=med_p, flasher=flasher, led=None,
                steps=steps, stop_detected=(mode == "stop"))


def expected_variant(key, mode):
    """clsimhip_get_table("kernel_variant") without its last entry (FAST)"""
    lengths, tilt, aniso, flasher = key
    return [float(LENGTHS.index(lengths)), float(tilt), float(aniso), float(flasher), 0.0 if mode == "stop" else 1.0]


def expected_launch(key, family, fast):
    """GetLastLaunch() of a launch of `family` for this key (table maker keys have three entries: its kernels always have the flasher)"""
    return dict(family=family, lengths=key[0], tilt=key[1], aniso=key[2], flasher=(key[3] if len(key) > 3 else True), fast=fast)
