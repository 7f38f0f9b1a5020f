"""Recipes for the per-trip mainline of the run-time compiled pooled kernel (round 9: tilt z index without the floor, distance bins
bounded by tilt_nd, the correction row's address and the layer's lower boundary read from table words).  Shared by
tests/test_baked_mainline.py (CPU: the recipes are what they claim, the oracle detects enough) and tests/test_baked_mainline_gpu.py
(pooled baked = pooled precompiled = oracle).  A plain module: no fixtures, nothing runs on import.

Every recipe is a tests/parity_recipes.py Recipe of N_STEPS steps whose first PLACED steps sit, on purpose, where the rewritten index
arithmetic could differ from the oracle's: on layer boundaries, below the first and above the last layer, below the tilt table's
first z and above its last, left of the first tilt distance, right of the last, exactly on every inner edge, and outside the string
proximity map on all four sides.  Their length is 0, so their photons are born exactly there.  The other steps are a cascade bunch
inside the detector, which is where the detected photons come from."""
import ctypes as C
import math

import numpy as np

from clsim_amd import _lib
from clsim_amd import converter as CV
from clsim_amd import synthetic as S
from oracle import builders as B
from tests import common
from tests import kernel_matrix as KM
from tests import parity_recipes as PR

N_STEPS = 1024
PLACED = 256
# name -> the instantiation its default launch takes: (lengths kind, tilt, anisotropy, flasher, FAST)
RECIPES = {
    "mie": ("icecube", True, False, False, True),
    "tilt_nd2": ("icecube", True, False, False, True),
    "tilt_nd3": ("icecube", True, False, False, True),
    "tilt_nd8": ("icecube", True, False, False, True),
    "constant_tilt": ("constant", True, False, False, True),
    "table_tilt": ("table", True, False, False, True),
    # SPICE-Mie with both refractive indices tabulated at 31 wavelengths: 62 words in front of the layer records, which then start
    # on no multiple of four words -- the run-time compiled kernel keeps the three-word read of the record plus its fourth word
    "mie_index_tables": ("icecube", True, False, False, True),
}
# (recipe, tuning "generic_kernels"): the generic instantiation keeps the per-bin proof test and the multiplied-out row address
CASES = [(name, 0) for name in RECIPES] + [("mie", 1), ("tilt_nd2", 1), ("tilt_nd8", 1)]


def synthetic_tilt(nd, zcoords):
    """nd distances 128 m apart (2: 1024 m) around the origin -- powers of two: every width's reciprocal is exact, so the FAST
    instantiation stays in reach -- over SPICE-Mie's z coordinates, with corrections of up to 30 m that depend on both indices"""
    dist = np.array([-512.0, 512.0]) if nd == 2 else 128.0 * (np.arange(nd) - (nd - 1) / 2.0)
    z = np.asarray(zcoords, dtype=np.float64)
    zcorr = np.array([[30.0 * math.sin(0.9 * j + 1.0) * math.cos(0.013 * zz + 0.4 * j) for zz in z] for j in range(nd)])
    return dict(distances=np.ascontiguousarray(dist), zcoords=np.ascontiguousarray(z), zcorr=np.ascontiguousarray(zcorr), azimuth=225.0 * B.DEG)


def media(name):
    """(med_o, med_p)"""
    if name == "constant_tilt":
        return KM.media(("constant", True, False, False))
    if name == "table_tilt":
        return KM.media(("table", True, False, False))
    directory = PR.ice_dir("spice_mie")
    med_o = B.load_ppc_ice(directory)
    if name == "mie":
        return med_o, PR.product_medium(directory=directory)
    if name == "mie_index_tables":
        # the photonics SPICE-Mie table's indices (30 wavelengths), one more value appended along the last step
        pho_o = B.load_photonics_ice(common.PHOTONICS["photonics_mie"])
        pho_p = CV.MakeIceCubeMediumPropertiesPhotonics(common.PHOTONICS["photonics_mie"])
        pho_d = _lib.MediumDesc()
        assert _lib.load().clsimhip_medium_describe(pho_p._h, C.byref(pho_d)) == 0
        tables, arrays = {}, []
        for key in ("phase", "group"):
            t = pho_o[key + "_table"]
            v = np.asarray(t["values"], dtype=np.float64)
            tables[key + "_table"] = dict(t, values=np.ascontiguousarray(np.append(v, 2.0 * v[-1] - v[-2])))
            arrays.append(tables[key + "_table"]["values"])
        assert len(arrays[0]) == len(arrays[1]) == 31

        def edit(d):
            d.phase_index_kind, d.group_index_kind = pho_d.phase_index_kind, pho_d.group_index_kind
            for key, values in zip(("phase", "group"), arrays):
                f = getattr(pho_d, key + "_index_table")
                f.n = len(values)
                f.values = values.ctypes.data_as(_lib.DP)
                setattr(d, key + "_index_table", f)
            return (arrays, pho_p)
        return dict(med_o, **tables), PR.product_medium(edit, directory)
    nd = int(name[len("tilt_nd"):])
    tilt = synthetic_tilt(nd, med_o["tilt"]["zcoords"])
    med_o = dict(med_o, tilt=tilt)
    flat = np.ascontiguousarray(tilt["zcorr"].ravel())

    def edit(d):
        d.has_tilt = 1
        d.tilt_num_distances, d.tilt_num_z = nd, len(tilt["zcoords"])
        d.tilt_distances = tilt["distances"].ctypes.data_as(_lib.DP)
        d.tilt_z_coordinates = tilt["zcoords"].ctypes.data_as(_lib.DP)
        d.tilt_z_corrections = flat.ctypes.data_as(_lib.DP)
        d.tilt_azimuth = tilt["azimuth"]
        return (tilt, flat)
    return med_o, PR.product_medium(edit, directory)


def f32(v):
    return np.float32(v)


def tilt_literals(med_o):
    """(lnx, lny, distances) as the float literals both sides hold (capi.make_tables, tables.cpp)"""
    t = med_o["tilt"]
    return f32(np.cos(t["azimuth"])), f32(np.sin(t["azimuth"])), np.asarray(t["distances"], dtype=np.float64).astype(np.float32)


def tilt_nr(lnx, lny, x, y):
    """the oracle's own arithmetic (oracle/clsim_oracle.c: nr = lnx * x + lny * y): two single precision products, then their sum"""
    return f32(f32(lnx * f32(x)) + f32(lny * f32(y)))


def xy_on_edge(lnx, lny, edge):
    """float32 (x, y) whose nr IS the float32 `edge`: searched among the neighbours of the real solution, for a few y"""
    edge = f32(edge)
    for y in (0.0, 1.0, -1.0, 0.5, 3.0, -7.0, 40.0):
        y = f32(y)
        x = f32((float(edge) - float(lny) * float(y)) / float(lnx))
        down = up = x
        for _ in range(256):
            for cand in (down, up):
                if tilt_nr(lnx, lny, cand, y) == edge:
                    return cand, y
            down, up = np.nextafter(down, f32(-np.inf)), np.nextafter(up, f32(np.inf))
    raise AssertionError("no float32 position with nr == %r" % edge)


def placed_positions(med_o):
    """[(x, y, z, what)]: the positions the issue names"""
    bottom, height, n = f32(med_o["layers_z_start"]), f32(med_o["layers_height"]), int(med_o["num_layers"])
    lnx, lny, dist = tilt_literals(med_o)
    zc = np.asarray(med_o["tilt"]["zcoords"], dtype=np.float64)
    first_z, dz = B.tilt_spacing(zc)
    last_z = first_z + dz * (len(zc) - 1)
    out = []
    for k in sorted({0, 1, n // 3, n // 2, n - 1, n}):
        # mediumLayerBoundary in float (c.cl:78-81): a product, then a sum
        out.append((30.0, -20.0, float(f32(f32(f32(k) * height) + bottom)), "layer boundary %d" % k))
    out.append((10.0, 15.0, float(bottom) - 30.0, "below the first layer"))
    out.append((10.0, 15.0, float(bottom) + n * float(height) + 30.0, "above the last layer"))
    for z, what in ((first_z - 25.0, "below the tilt table"), (first_z, "the tilt table's first z"), (last_z, "the tilt table's last z"),
                    (last_z + 25.0, "above the tilt table")):
        out.append((-40.0, 25.0, z, what))
    for nr, what in ((float(dist[0]) - 50.0, "left of the first tilt distance"), (float(dist[-1]) + 50.0, "right of the last tilt distance")):
        out.append((nr * float(lnx), nr * float(lny), 0.0, what))
    for j in range(len(dist)):
        x, y = xy_on_edge(lnx, lny, dist[j])
        out.append((float(x), float(y), 12.5, "tilt distance %d" % j))
    for x, y, what in ((-2500.0, 0.0, "west"), (2500.0, 0.0, "east"), (0.0, -2500.0, "south"), (0.0, 2500.0, "north"), (2500.0, -2500.0, "corner")):
        out.append((x, y, -100.0, "outside the string map: " + what))
    return out


def steps_for(med_o, seed):
    steps = S.cascade_steps(N_STEPS, seed=seed, pad_to=256)
    assert len(steps) == N_STEPS
    positions = placed_positions(med_o)
    assert 4 * len(positions) <= PLACED
    for i in range(PLACED):
        x, y, z, _ = positions[i % len(positions)]
        steps["x"][i], steps["y"][i], steps["z"][i] = x, y, z
        steps["length"][i] = 0.0
        # (straight down and straight up among the random directions: the walk's two signs from a boundary)
        if (i // len(positions)) == 1:
            steps["theta"][i] = np.float32(np.pi)
        elif (i // len(positions)) == 2:
            steps["theta"][i] = 0.0
    return steps


_recipes = {}


def recipe(name):
    if name not in _recipes:
        med_o, med_p = media(name)
        steps = steps_for(med_o, seed=211 + list(RECIPES).index(name))
        geom = common.config("mie")["geom"]
        R = PR.custom(name, med_o, med_p, geom, PR.cherenkov_o(med_o), PR.cherenkov_p(med_p), steps)
        R.med_o = med_o
        _recipes[name] = R
    return _recipes[name]


_compiled = {}


def compiled(name):
    """the recipe's converter after Compile() (host only), made once: tuning a test changes on it, it puts back"""
    if name not in _compiled:
        _compiled[name] = recipe(name).make_converter(initialize=False)
    return _compiled[name]
