"""The ad-hoc configurations of tests/test_parity_gpu.py as recipes, built on both sides: the oracle's tables and the product's
converter.  tests/test_parity_gpu.py (classic kernel, default tuning) and tests/test_baked_switches_gpu.py (pooled kernel,
precompiled and compiled at run time with the configuration as literals) share them; tests/test_kernel_matrix.py compiles them on
the CPU.  A plain module: no fixtures, nothing runs on import.

A recipe is a Recipe: `T` the oracle's tables, `steps` the bunch, `streams` the (x, a) both sides start from, and
`make_converter(tuning=None, initialize=True)`, which goes through CV.initializeHIP(..., tuning=tuning) -- or, with initialize=False,
stops after Compile() (host only: what the CPU guard compiles)."""
import ctypes as C
import os

import numpy as np

from clsim_amd import _lib
from clsim_amd import converter as CV
from clsim_amd import synthetic as S
from oracle import builders as B
from oracle import capi
from tests import common


class Recipe:
    def __init__(self, name, T, steps, streams, make_converter):
        self.name, self.T, self.steps, self.streams, self.make_converter = name, T, steps, streams, make_converter


def _converter_factory(geometry, med_p, bias_p, gens_p, n, streams, **options):
    """make_converter of a recipe: geometry is a callable (a text-file geometry is read when the converter is made)"""
    def make_converter(tuning=None, initialize=True):
        if initialize:
            return CV.initializeHIP(0, geometry(), med_p, bias_p, gens_p, approximateNumberOfWorkItems=n, streams=streams, tuning=tuning,
                                    **options)
        # the configuration sequence of CV.initializeHIP up to Compile(): no device is touched
        conv = CV.I3CLSimStepToPhotonConverterHIP(0)
        for key, value in (tuning or {}).items():
            conv.SetTuning(key, value)
        conv.SetWlenGenerators(gens_p); conv.SetWlenBias(bias_p); conv.SetMediumProperties(med_p); conv.SetGeometry(geometry())
        conv.SetStopDetectedPhotons(True)
        conv.SetFixedNumberOfAbsorptionLengths(options.get("fixedNumberOfAbsorptionLengths", float("nan")))
        conv.SetDOMPancakeFactor(options.get("pancakeFactor", 1.0))
        conv.Compile()
        return conv
    return make_converter


def custom(name, med_o, med_p, geom, gens_o, gens_p, steps, pancake=5.0, max_items=None, bias_o=None, bias_p=None, fixed_abs_lengths=None,
           product_geometry=None):
    """An ad-hoc configuration: gens_o(bias) / gens_p(bias) give the wavelength generators of either side (the default bias is the
    IceCube DOM acceptance); geom is the oracle's geometry dict, product_geometry() the product's where it is not made from that dict."""
    n = len(steps)
    streams = common.streams(max_items or n)
    geo = B.build_geometry(geom["string_ids"], geom["dom_ids"], geom["x"], geom["y"], geom["z"], geom["subdetectors"], geom["om_radius"])
    bias_o = B.icecube_dom_acceptance() if bias_o is None else bias_o
    extra_o = {} if fixed_abs_lengths is None else dict(fixed_abs_lengths=fixed_abs_lengths)
    T = capi.make_tables(med_o, geo, gens_o(bias_o), bias_o, pancake=pancake, **extra_o)
    bias_p = CV.GetIceCubeDOMAcceptance() if bias_p is None else bias_p
    options = dict(pancakeFactor=pancake)
    if fixed_abs_lengths is not None:
        options["fixedNumberOfAbsorptionLengths"] = fixed_abs_lengths
    geometry = product_geometry or (lambda: CV.I3CLSimSimpleGeometry.from_dict(geom))
    return Recipe(name, T, steps, streams, _converter_factory(geometry, med_p, bias_p, gens_p(bias_p), n, streams, **options))


def ice_dir(model):
    return os.path.join(common.ICE, model)


def cherenkov_o(med_o):
    return lambda bias: [B.cherenkov_wlen_generator(bias, med_o)]


def cherenkov_p(med_p):
    return lambda bias: [CV.makeCherenkovWavelengthGenerator(bias, med_p)]


def product_medium(desc_edit=None, directory=None, tilt=True):
    med = CV.MakeIceCubeMediumProperties(iceDataDirectory=directory, useTiltIfAvailable=tilt)
    if desc_edit is None:
        return med
    d = _lib.MediumDesc()
    assert _lib.load().clsimhip_medium_describe(med._h, C.byref(d)) == 0
    keep = desc_edit(d)
    h = C.c_void_p()
    assert _lib.load().clsimhip_medium_create(C.byref(d), C.byref(h)) == 0
    return CV.I3CLSimMediumProperties(h, keep=(med, keep))


VARIANTS = ("no_pancake", "no_tilt", "single_icecube_layer", "hg_only", "liu_only", "lea_no_tilt", "flasher_c1", "table_float",
            "table_with_tilt_and_aniso", "no_dispersion_no_bias", "group_velocity_from_dispersion")


def variant_steps():
    return common.steps_for(common.config("mie"), 2048, seed=31)


def variant(kind):
    """Variants of the generated program: PANCAKE_FACTOR undefined (pancake = 1), getTiltZShift_IS_CONSTANT with
    layered ice (carried layer index), a one-layer IceCube medium (un-optimised per-function form, SURVEY 9.7 ii),
    pure HG / pure Liu scattering, anisotropy without tilt, flasher generator with constant-length medium."""
    geom = S.ic86_geometry()
    steps = variant_steps()
    if kind == "no_pancake":
        med_o = B.load_ppc_ice(ice_dir("spice_mie"))
        med_p = product_medium(directory=ice_dir("spice_mie"))
        return custom(kind, med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps, pancake=1.0)
    if kind == "no_tilt":
        med_o = B.load_ppc_ice(ice_dir("spice_mie"), use_tilt_if_available=False)
        med_p = product_medium(directory=ice_dir("spice_mie"), tilt=False)
        return custom(kind, med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps)
    if kind == "lea_no_tilt":
        med_o = B.load_ppc_ice(ice_dir("spice_lea"), use_tilt_if_available=False)
        med_p = product_medium(directory=ice_dir("spice_lea"), tilt=False)
        return custom(kind, med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps)
    if kind == "group_velocity_from_dispersion":
        # no group refractive index override: getGroupVelocity from the phase index and its derivative
        # (I3CLSimHelperGenerateMediumPropertiesSource.cxx:274-300); every arrival time moves by up to 1 %
        cfg = common.config("lea_dispersion")
        med_o, med_p = cfg["med_o"], cfg["med_p"]
        return custom(kind, med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps)
    if kind == "no_dispersion_no_bias":
        # generateCherenkovPhotonsWithoutDispersion with a constant bias of 1 (ModuleHelper.cxx:265-275):
        # I3CLSimRandomValueWlenCherenkovNoDispersion over the medium's wavelength range, constant wavelength bias
        med_o = B.load_ppc_ice(ice_dir("spice_mie"))
        med_p = product_medium(directory=ice_dir("spice_mie"))
        return custom(kind, med_o, med_p, geom,
                      lambda bias: [dict(kind="nodispersion", **{"from": med_o["min_wlen"], "to": med_o["max_wlen"]})],
                      lambda bias: [CV.I3CLSimRandomValueWlenCherenkovNoDispersion(med_o["min_wlen"], med_o["max_wlen"])], steps,
                      bias_o=dict(kind="const", value=1.0), bias_p=CV.I3CLSimFunctionConstant(1.0))
    if kind in ("table_float", "table_with_tilt_and_aniso"):
        # per-layer FromTable lengths stored as floats (storeDataAsHalfPrecision=False); and tabulated lengths under
        # the tilt / anisotropy / Mixed scattering objects of SPICE-Lea (no reference loader builds this mix, the classes allow it)
        path = common.PHOTONICS["photonics_mie"]
        med_o = B.load_photonics_ice(path)
        lea_o = B.load_ppc_ice(ice_dir("spice_lea"))
        lea_p = CV.MakeIceCubeMediumProperties(iceDataDirectory=ice_dir("spice_lea"))
        lea_d = _lib.MediumDesc()
        assert _lib.load().clsimhip_medium_describe(lea_p._h, C.byref(lea_d)) == 0
        if kind == "table_float":
            med_o["table"]["store16"] = False
        else:
            for key in ("aniso", "pre", "post", "tilt"):
                med_o[key] = lea_o[key]
            med_o["scat"] = lea_o["scat"]
        tab = CV.MakeIceCubeMediumPropertiesPhotonics(path)
        d = _lib.MediumDesc()
        assert _lib.load().clsimhip_medium_describe(tab._h, C.byref(d)) == 0
        if kind == "table_float":
            d.table_store_as_16bit = 0
        else:
            for f in ("scatter_kind", "liu_fraction", "mean_cosine", "has_anisotropy", "aniso_azimuth", "aniso_k1", "aniso_k2",
                      "has_pre_transform", "pre_renormalize", "pre_matrix", "has_post_transform", "post_renormalize", "post_matrix",
                      "has_tilt", "tilt_num_distances", "tilt_num_z", "tilt_distances", "tilt_z_coordinates", "tilt_z_corrections",
                      "tilt_azimuth"):
                setattr(d, f, getattr(lea_d, f))
        h = C.c_void_p()
        assert _lib.load().clsimhip_medium_create(C.byref(d), C.byref(h)) == 0
        med_p = CV.I3CLSimMediumProperties(h, keep=(tab, lea_p))
        return custom(kind, med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps)
    if kind in ("hg_only", "liu_only"):
        med_o = B.load_ppc_ice(ice_dir("spice_mie"))
        med_o["scat"]["kind"] = "hg" if kind == "hg_only" else "liu"

        def edit(d):
            d.scatter_kind = 0 if kind == "hg_only" else 1
        med_p = product_medium(edit, ice_dir("spice_mie"))
        return custom(kind, med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps)
    if kind == "single_icecube_layer":
        full = B.load_ppc_ice(ice_dir("spice_mie"), use_tilt_if_available=False)
        med_o = dict(full, num_layers=1, layers_z_start=-1000.0, layers_height=2000.0,
                     aDust400=full["aDust400"][85:86], deltaTau=full["deltaTau"][85:86], b400=full["b400"][85:86])
        arrays = [np.ascontiguousarray(med_o[k], dtype=np.float64) for k in ("aDust400", "deltaTau", "b400")]

        def edit(d):
            d.num_layers = 1; d.layers_z_start = -1000.0; d.layers_height = 2000.0
            d.a_dust400, d.delta_tau, d.b400 = (a.ctypes.data_as(_lib.DP) for a in arrays)
            return arrays
        med_p = product_medium(edit, ice_dir("spice_mie"), tilt=False)
        return custom(kind, med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps)
    assert kind == "flasher_c1", kind
    # constant lengths + second (constant) generator, single string
    g1 = S.single_string_geometry()
    med_o = B.homogeneous_medium()
    med_p = CV.MakeHomogeneousMediumProperties()
    st = S.flasher_steps(1024, seed=4, position=(30.0, 20.0, 100.0), pad_to=256)
    st["sourceType"][:100] = 0          # a few Cherenkov steps in the same bunch
    st["length"][:100] = 0.001
    st["num"][100:120] = 0              # and a few empty ones
    return custom(kind, med_o, med_p, g1, lambda bias: [B.cherenkov_wlen_generator(bias, med_o), dict(kind="const", value=405e-9)],
                  lambda b: [CV.makeCherenkovWavelengthGenerator(b, med_p), CV.I3CLSimRandomValueConstant(405e-9)], st)


def fixed_number_of_absorption_lengths():
    """PROPAGATE_FOR_FIXED_NUMBER_OF_ABSORPTION_LENGTHS with 1.75 lengths, SPICE-Mie in IC86"""
    cfg = common.config("mie")
    steps = common.steps_for(cfg, 2048, seed=17)
    return custom("fixed_abs_lengths", cfg["med_o"], cfg["med_p"], cfg["geom"], cherenkov_o(cfg["med_o"]), cherenkov_p(cfg["med_p"]), steps,
                  fixed_abs_lengths=1.75)


def text_file_geometry_single_subdetector(directory):
    """geometry read from an I3CLSimSimpleGeometryTextFile-format file written into `directory`: all 86 strings in the one
    subdetector "default", i.e. a single fine cell grid instead of the IceCube / DeepCore pair"""
    g = S.ic86_geometry()
    path = os.path.join(str(directory), "geo.txt")
    with open(path, "w") as f:
        for i in range(len(g["x"])):
            f.write("%d %d %.17g %.17g %.17g\n" % (g["string_ids"][i], g["dom_ids"][i], g["x"][i], g["y"][i], g["z"][i]))
    cfg = common.config("mie")
    steps = common.steps_for(cfg, 2048, seed=8)
    go = B.geometry_from_text_file(path, g["om_radius"])
    return custom("text_file_geometry", cfg["med_o"], cfg["med_p"], go, cherenkov_o(cfg["med_o"]), cherenkov_p(cfg["med_p"]), steps,
                  product_geometry=lambda: CV.I3CLSimSimpleGeometry.from_text_file(g["om_radius"], path))


def range_restricted_divides(n_steps=3072):
    """SPICE-Mie without tilt; the first third of the steps makes photons EXACTLY on a layer boundary and heading down, the second
    third belongs to a particle below the Cherenkov threshold (tests/test_parity_gpu.py:
    test_range_restricted_divides_fall_back_to_the_ieee_sequence).  Returns (recipe, med_o, the heights of the first third)."""
    third = n_steps // 3
    ice = ice_dir("spice_mie")
    med_o = B.load_ppc_ice(ice, use_tilt_if_available=False)
    med_p = CV.MakeIceCubeMediumProperties(iceDataDirectory=ice, useTiltIfAvailable=False)
    geom = S.ic86_geometry()
    steps = common.steps_for(common.config("mie"), n_steps, seed=77)
    bottom, height = np.float32(med_o["layers_z_start"]), np.float32(med_o["layers_height"])
    k = np.arange(third) % 120 + 25
    on_boundary = (k.astype(np.float32) * height) + bottom                      # mediumLayerBoundary, c.cl:78-81, in float
    steps["z"][:third] = on_boundary
    steps["length"][:third] = 0.0                                               # photons are born at the step's start
    steps["theta"][:third] = np.float32(np.pi)                                  # heading down
    steps["beta"][third:2 * third] = 0.5
    return custom("range_restricted_divides", med_o, med_p, geom, cherenkov_o(med_o), cherenkov_p(med_p), steps), med_o, on_boundary


def detector_of_576_strings(n_steps=4096):
    """a table image beyond the budget of seven workgroups per CU (tables.cpp: compile_tables)"""
    cfg = dict(common.config("mie"))
    cfg["geom"] = S.large_detector_geometry()
    steps = S.cascade_steps(n_steps, seed=17, radius=1400.0)
    return custom("detector_of_576_strings", cfg["med_o"], cfg["med_p"], cfg["geom"], cherenkov_o(cfg["med_o"]), cherenkov_p(cfg["med_p"]), steps)


def named(name, n_steps, seed=3):
    """a configuration of tests/common.py with its steps, as tests/test_parity_gpu.py: run_both builds it"""
    cfg = common.config(name)
    steps = common.steps_for(cfg, n_steps, seed=seed)
    bias_o = B.icecube_dom_acceptance()
    bias_p = CV.GetIceCubeDOMAcceptance()
    return custom(name, cfg["med_o"], cfg["med_p"], cfg["geom"], lambda bias: common.oracle_generators(cfg, bias),
                  lambda bias: common.product_generators(cfg, bias), steps, bias_o=bias_o, bias_p=bias_p)


# ---- one recipe per value of a configuration switch the pooled kernel can see (KParams members that the run-time compiled kernel takes
# as literals): tests/test_baked_switches_gpu.py runs them, tests/test_kernel_matrix.py compiles them.  Bunches of 1 024 ... 2 048 steps.
# name -> (factory(directory), what the recipe is there for)
SWITCHES = {
    "no_pancake": (lambda d: variant("no_pancake"), "has_pancake = 0"),
    "hg_only": (lambda d: variant("hg_only"), "scatter_kind: Henyey-Greenstein only"),
    "liu_only": (lambda d: variant("liu_only"), "scatter_kind: simplified Liu only"),
    "single_icecube_layer": (lambda d: variant("single_icecube_layer"), "num_layers = 1"),
    "no_dispersion_no_bias": (lambda d: variant("no_dispersion_no_bias"), "gen_kind = 2 (no dispersion), bias_kind = 1 (constant)"),
    "flasher_c1": (lambda d: variant("flasher_c1"), "gen_kind = 1 (constant wavelength), constant lengths, one string"),
    "flasher_led405": (lambda d: named("flasher_led405", 2048), "gen_kind = 3 (a table with its own wavelengths)"),
    "photonics_mie": (lambda d: named("photonics_mie", 2048), "phase_kind, group_kind: tables; the generic instantiation"),
    "photonics_wham": (lambda d: named("photonics_wham", 2048), "phase_kind, group_kind: tables; the generic instantiation"),
    "group_velocity_from_dispersion": (lambda d: variant("group_velocity_from_dispersion"), "group_kind: dispersion; the generic instantiation"),
    "table_float": (lambda d: variant("table_float"), "length table stored as float"),
    "fixed_abs_lengths": (lambda d: fixed_number_of_absorption_lengths(), "has_fixed_abs = 1"),
    "text_file_geometry": (lambda d: text_file_geometry_single_subdetector(d), "num_subdet = 1"),
    "ic86": (lambda d: named("mie", 2048), "num_subdet = 2: IC86 as it is"),
    "mie_regular": (lambda d: named("mie_regular", 2048), "DOM position templates shared by the strings and small enough for LDS: dom_in_lds = 1"),
    "detector_of_576_strings": (lambda d: detector_of_576_strings(2048), "dom_in_lds = 0 (as IC86: one template per string stays in global memory) with an image beyond seven workgroups per CU"),
    "range_restricted_divides": (lambda d: range_restricted_divides(1536)[0], "div_ok without the tilt's bit; steps on layer boundaries and below the Cherenkov threshold"),
}

# the instantiation each switch recipe compiles to: (lengths kind, tilt, anisotropy, flasher, FAST).  FAST exists for Mixed scattering,
# an overridden group index and proven divisions only (tables.cpp: medium_proofs_complete), so pure HG / Liu, the photonics tables and
# the group velocity from dispersion reach the generic instantiations without "generic_kernels".
SWITCH_INSTANTIATIONS = {
    "no_pancake": ("icecube", True, False, False, True),
    "hg_only": ("icecube", True, False, False, False),
    "liu_only": ("icecube", True, False, False, False),
    "single_icecube_layer": ("icecube", False, False, False, True),
    "no_dispersion_no_bias": ("icecube", True, False, False, True),
    "flasher_c1": ("constant", False, False, True, True),
    "flasher_led405": ("icecube", True, True, True, True),
    "photonics_mie": ("table", False, False, False, False),
    "photonics_wham": ("table", False, False, False, False),
    "group_velocity_from_dispersion": ("icecube", True, True, False, False),
    "table_float": ("table", False, False, False, False),
    "fixed_abs_lengths": ("icecube", True, False, False, True),
    "text_file_geometry": ("icecube", True, False, False, True),
    "ic86": ("icecube", True, False, False, True),
    "mie_regular": ("icecube", True, False, False, True),
    "detector_of_576_strings": ("icecube", True, False, False, True),
    "range_restricted_divides": ("icecube", False, False, False, True),
}
