"""Recipes for the layer-crossing loop of the run-time compiled pooled kernel (round 10: signed running sums, one induction variable,
the crossed layer's record in one read, two-instruction index clamps).  Shared by tests/test_walk_loop_gpu.py (pooled baked = pooled
precompiled = oracle) and its guard, which runs on the CPU before the GPU is touched.  A plain module: nothing runs on import.

Every recipe is a tests/parity_recipes.py Recipe of N_STEPS steps.  The first PLACED steps are placed by hand; the rest is a cascade
bunch inside the detector, which is where the detected photons come from.  A placed step has length 0 and beta = 0.5: below the
Cherenkov threshold the reference emits the photon along the step (cosCherenkov = min(1, 1 / (beta n)) = 1), so every photon of the
step is born at the step's position with the step's direction, whatever its random numbers are.  placed_steps() lists what is placed.

What the oracle cannot report -- how many layers a trip crosses and where its walk ends -- is restated here in numpy for the FIRST
trip of every photon of a placed step (first_trips): single precision, operation by operation, oracle/clsim_oracle.c:1014-1047.
The random numbers of that trip come from the oracle alone: a step's photons draw from the step's stream one after the other, so the
stream's state when photon m is created is the state the oracle returns for the same step with ONE photon started from the state of
photon m - 1 (prefix_states; the last of them must be the state the whole bunch leaves behind, which the guard asserts).  Wavelength,
logarithm, tilt shift and the layers' lengths are the oracle's own functions (capi.sample, eval_math, eval_field, eval_medium)."""
import numpy as np

from oracle import builders as B
from oracle import capi
from clsim_amd import synthetic as S
from tests import baked_mainline as BM
from tests import common
from tests import parity_recipes as PR

N_STEPS = 1024
PLACED = 256
PLACED_PHOTONS = 384            # photons of a placed step (constant lengths: a sixth fewer five-layer trips than SPICE-Mie per photon)
# name -> the instantiation its default launch takes: (lengths kind, tilt, anisotropy, flasher, FAST)
RECIPES = {
    "mie": ("icecube", True, False, False, True),
    "constant_tilt": ("constant", True, False, False, True),
    "table_tilt": ("table", True, False, False, True),
    "mie_no_tilt": ("icecube", False, False, False, True),
    # layer records on no multiple of four words: the three-word read in the loop (tests/baked_mainline.py)
    "mie_index_tables": ("icecube", True, False, False, True),
}
# (recipe, tuning "generic_kernels")
CASES = [(name, 0) for name in RECIPES] + [("mie", 1)]
EPSILON = np.float32(0.00001)
F = np.float32


def media(name):
    if name == "mie_no_tilt":
        directory = PR.ice_dir("spice_mie")
        return B.load_ppc_ice(directory, use_tilt_if_available=False), PR.product_medium(directory=directory, tilt=False)
    return BM.media(name)


def layers_of(med_o):
    return F(med_o["layers_z_start"]), F(med_o["layers_height"]), int(med_o["num_layers"])


def boundary(med_o, k):
    """mediumLayerBoundary in float (c.cl:78-81): a product, then a sum"""
    bottom, height, _ = layers_of(med_o)
    return F(F(F(k) * height) + bottom)


def z_for_effective(T, x, y, z_eff):
    """a z whose effective height z - tiltZShift(x, y, z) is z_eff to within the shift's own variation over a few centimetres"""
    z = float(z_eff)
    if T.t.has_tilt:
        for _ in range(6):
            z = float(z_eff) + float(capi.eval_field(T, 0, [[x, y, z]])[0])
    else:
        z = float(z_eff) + float(T.t.tilt_const)
    return z


def clearest_layers(T, med_o, count=6):
    """[(layer, direction)]: the starts, away from both ends, from whose far boundary the next four layers in that direction (+1 up,
    -1 down) hold the fewest scattering lengths at 400 nm -- where a vertical photon most often crosses five boundaries in one trip"""
    _, height, n = layers_of(med_o)
    per_layer = float(height) / np.array([capi.eval_medium(T, 1, [4.0e-7], layer)[0] for layer in range(n)], dtype=np.float64)
    cost = sorted([(per_layer[k + 1:k + 5].sum(), k, 1) for k in range(30, n - 30)] + [(per_layer[k - 4:k].sum(), k, -1) for k in range(30, n - 30)])
    return [(k, d) for _, k, d in cost[:count]]


def placed_steps(T, med_o):
    """[(x, y, z, theta, what)] for the PLACED steps.  theta is the polar angle of the direction of flight: 0 is up."""
    bottom, height, n = layers_of(med_o)
    h = float(height)
    up, down = 0.0, float(F(np.pi))
    half_pi = F(np.pi / 2)
    out = []

    def centre(layer):
        return float(bottom) + (layer + 0.5) * h

    def add(x, y, z_eff, theta, what):
        out.append((x, y, z_for_effective(T, x, y, z_eff), float(theta), what))

    # starts in layer 0 heading down and in the last layer heading up: the loop's "last layer" test is true on entry
    for i in range(6):
        add(40.0 + 7.0 * i, -35.0, centre(0) + 0.4 * i, down - 2.0e-4 * i, "layer 0 heading down")
        add(-60.0, 20.0 + 9.0 * i, centre(n - 1) - 0.4 * i, up + 2.0e-4 * i, "last layer heading up")
    # one and two layers from either end, heading for it: the last layer is reached in mid-walk
    for i in range(4):
        for k in (1, 2):
            # (a centimetre or two from the boundary they head for: the first crossing is all but certain)
            add(15.0 * i, 25.0, float(boundary(med_o, k)) + 0.01 * (i + 1), down - 3.0e-4 * i, "%d from the bottom heading down" % k)
            add(-15.0 * i, -45.0, float(boundary(med_o, n - k)) - 0.01 * (i + 1), up + 3.0e-4 * i, "%d from the top heading up" % k)
    # dz around zero: as close to +0 and -0 as a polar angle gets (the neighbours of pi / 2), +-5e-6 (below kEpsilon), +-2e-5 (above)
    clear = clearest_layers(T, med_o)
    for i, theta in enumerate((half_pi, np.nextafter(half_pi, F(0)), np.nextafter(half_pi, F(4)), F(half_pi - F(5e-6)), F(half_pi + F(5e-6)),
                               F(half_pi - F(2e-5)), F(half_pi + F(2e-5)))):
        for k in (0, 1):
            # 2 cm above a boundary / below it: a flat photon 20 000 m from the boundary along its path
            add(120.0 - 30.0 * i, 80.0, float(boundary(med_o, clear[k][0] + k)) + (0.02 if k == 0 else -0.02), theta, "dz around zero")
    # length-0 steps exactly on layer boundaries (round 9's placement: the boundary is the photon's z, not its effective z), down and up
    for k in sorted({0, 1, n // 3, n // 2, n - 1, n}):
        for theta in (down, up):
            out.append((30.0, -20.0, float(boundary(med_o, k)), theta, "on layer boundary %d" % k))
    # a millimetre in front of a boundary of the dustiest layers: the first crossing is certain, and the absorption budget of a share of
    # the photons ends inside the layer they cross into
    sca = np.array([capi.eval_medium(T, 0, [4.0e-7], layer)[0] for layer in range(n)])
    inner = np.arange(30, n - 30)
    dusty = [int(k) for k in inner[np.argsort(sca[inner], kind="stable")[:4]]]
    for i, k in enumerate(dusty):
        for j in range(3):
            add(-100.0 + 20.0 * j, 10.0 * i, float(boundary(med_o, k + 1)) + 0.001, down, "just above a dusty layer heading down")
            add(100.0 - 20.0 * j, -10.0 * i, float(boundary(med_o, k)) - 0.001, up, "just below a dusty layer heading up")
    # the rest: within 1e-3 of +-z in the clearest layers, so that walks are long
    i = 0
    while len(out) < PLACED:
        k, direction = clear[i % len(clear)]
        tilt_off = (0.0, 2.5e-4, 5.0e-4, 9.0e-4)[(i // len(clear)) % 4]
        theta = (down - tilt_off) if direction < 0 else (up + tilt_off)
        # (a few centimetres in front of the layer's far boundary, so that the fifth crossing is four layers away)
        z_eff = float(boundary(med_o, k + 1)) - 0.01 * (1 + i % 7) if direction > 0 else float(boundary(med_o, k)) + 0.01 * (1 + i % 7)
        add(-200.0 + 37.0 * (i % 11), -150.0 + 29.0 * (i % 13), z_eff, theta, "near vertical in a clear layer")
        i += 1
    assert len(out) == PLACED
    return out


def steps_for(T, med_o, seed):
    steps = S.cascade_steps(N_STEPS, seed=seed, pad_to=256)
    assert len(steps) == N_STEPS
    placed = placed_steps(T, med_o)
    for i, (x, y, z, theta, _) in enumerate(placed):
        steps["x"][i], steps["y"][i], steps["z"][i] = x, y, z
        steps["theta"][i], steps["phi"][i] = theta, 0.37 * i
        steps["length"][i] = 0.0
        steps["beta"][i] = 0.5                      # below the Cherenkov threshold: the photon flies along the step
        steps["num"][i] = PLACED_PHOTONS
    return steps, [p[4] for p in placed]


_recipes = {}


def recipe(name):
    if name not in _recipes:
        med_o, med_p = media(name)
        geom = common.config("mie")["geom"]
        seed = 311 + list(RECIPES).index(name)
        # (the steps are placed with the oracle's own tables, which the recipe makes: a cascade bunch first, the placed steps then)
        R = PR.custom(name, med_o, med_p, geom, PR.cherenkov_o(med_o), PR.cherenkov_p(med_p), S.cascade_steps(N_STEPS, seed=seed, pad_to=256))
        R.steps, what = steps_for(R.T, med_o, seed)
        R.med_o, R.placed_what = med_o, what
        _recipes[name] = R
    return _recipes[name]


_compiled = {}


def compiled(name):
    if name not in _compiled:
        _compiled[name] = recipe(name).make_converter(initialize=False)
    return _compiled[name]


# ---- the first trip of every photon of the placed steps, restated ----

def prefix_states(T, steps, x, a):
    """states[m][i]: the state of placed step i's stream when its photon m is created.  A photon takes nothing over from the one before
    it but the stream, so this is the oracle's final state for the step with one photon, started from states[m - 1][i].
    states[PLACED_PHOTONS] is then the state the full bunch leaves behind (the caller compares)."""
    st = steps[:PLACED].copy()
    st["num"] = 1
    states = [np.array(x[:PLACED], dtype=np.uint64, copy=True)]
    for m in range(PLACED_PHOTONS):
        _, _, x_after, _ = capi.propagate(T, st, states[-1], a[:PLACED], max_hits=PLACED + 1)
        states.append(x_after)
    return states


def uniform_draws(x, a, draws):
    """rand_MWC_co (mwcrng_kernel.cl:12-20) for every stream: x = lo32(x) * a + hi32(x), u = float_rtz(lo32(x)) / 2^32, `draws` times.
    Returns (u [draw][stream], states).  guard() holds it against the oracle's own generator."""
    x = np.array(x, dtype=np.uint64, copy=True)
    a = np.asarray(a, dtype=np.uint64)
    out = np.empty((draws, len(x)), dtype=np.float32)
    for d in range(draws):
        x = (x & np.uint64(0xffffffff)) * a + (x >> np.uint64(32))
        lo = (x & np.uint64(0xffffffff)).astype(np.int64)
        # round toward zero to 24 significant bits: clear what lies below them, then the conversion is exact
        shift = np.maximum(np.floor(np.log2(np.maximum(lo, 1))).astype(np.int64) - 23, 0)
        out[d] = (((lo >> shift) << shift).astype(np.float64) * 2.0 ** -32).astype(np.float32)
    return out, x


def minus_log(u):
    return -capi.eval_math(0, np.asarray(u, dtype=np.float32))


def first_trips(T, med_o, steps, x, a, states=None):
    """For every photon of the placed steps, its first trip's walk: dict of arrays of shape (PLACED, PLACED_PHOTONS) --
    start (layer the walk starts in), end (layer it ends in), crossings, absorbed (the absorption budget ran out before the scattering
    budget: to_absorption < distance), dz."""
    assert not T.t.has_abs_corr and not T.t.has_fixed_abs
    states = prefix_states(T, steps, x, a) if states is None else states
    bottom, thickness, n = F(T.t.layer_bottom), F(T.t.layer_thickness), int(T.t.num_layers)
    recip_thickness = F(1.0) / thickness
    st = steps[:PLACED]
    a = np.ascontiguousarray(a[:PLACED], dtype=np.uint32)
    # the step's direction (oracle/clsim_oracle.c:962-969) and the photon's: cosa = 1, sina = 0 leaves it, then it is renormalised (:473-495)
    ct = capi.eval_math(3, st["theta"])
    sin_t = capi.eval_math(2, st["theta"])
    dx, dy = sin_t * capi.eval_math(3, st["phi"]), sin_t * capi.eval_math(2, st["phi"])
    sinth = capi.eval_math(8, np.maximum(F(0), F(1) - ct * ct))
    vertical = ~(sinth > 0)
    dx, dy = np.where(vertical, F(0), dx), np.where(vertical, F(0), dy)
    dz = np.where(vertical, np.sign(ct).astype(np.float32), ct)
    dz = (dz * capi.eval_math(7, (dx * dx + dy * dy) + dz * dz)).astype(np.float32)
    # the photon's position is the step's (length 0), so its effective height and first layer are the same for all photons of a step
    pos = np.stack([st["x"], st["y"], st["z"]], axis=1).astype(np.float32)
    if T.t.has_tilt:
        effective_z = (pos[:, 2] - capi.eval_field(T, 0, pos)).astype(np.float32)
        layer_of = effective_z
    else:
        effective_z = (pos[:, 2] - F(T.t.tilt_const)).astype(np.float32)
        layer_of = pos[:, 2]                        # (the carried layer is taken from z itself, c.cl:571-573)
    quotient = ((layer_of - bottom) / thickness).astype(np.float32)
    first = np.clip(np.where(np.isnan(quotient), 0, np.trunc(quotient)), 0, n - 1).astype(np.int64)
    # every photon's draws, in the order of createPhotonFromTrack and the loop's head: shift, wavelength, azimuth, absorption, scattering
    wlen = np.empty((PLACED_PHOTONS, PLACED), dtype=np.float32)
    u_abs, u_sca = np.empty_like(wlen), np.empty_like(wlen)
    for m in range(PLACED_PHOTONS):
        _, s = uniform_draws(states[m], a, 1)
        w, s = capi.sample(T, "wavelength", s, a, 1)
        u, s = uniform_draws(s, a, 3)
        wlen[m], u_abs[m], u_sca[m] = w[:, 0], u[1], u[2]
    shape = wlen.shape
    abs_lens_left = minus_log(F(1) - u_abs.ravel())
    sca_step_left = minus_log(F(1) - u_sca.ravel())
    flat_wlen = wlen.ravel()
    lengths = {}

    def lengths_in(layers):
        """(scattering, absorption) length of every lane in the layer it is in: a layer's lengths are asked of the oracle when some lane gets there"""
        sca_, abs_ = np.empty(flat_wlen.size, dtype=np.float32), np.empty(flat_wlen.size, dtype=np.float32)
        for layer in np.unique(layers):
            if layer not in lengths:
                lengths[layer] = (capi.eval_medium(T, 1, flat_wlen, int(layer)), capi.eval_medium(T, 0, flat_wlen, int(layer)))
            sel = layers == layer
            sca_[sel], abs_[sel] = lengths[layer][0][sel], lengths[layer][1][sel]
        return sca_, abs_
    dzp, eff, j0 = np.tile(dz, PLACED_PHOTONS), np.tile(effective_z, PLACED_PHOTONS), np.tile(first, PLACED_PHOTONS)
    down = dzp < 0
    lower = ((j0.astype(np.float32) * thickness).astype(np.float32) + bottom).astype(np.float32)
    b = np.where(down, lower, (lower + thickness).astype(np.float32)).astype(np.float32)
    j = j0.copy()
    cur_sca, cur_abs = lengths_in(j)
    ais = (((dzp * sca_step_left).astype(np.float32) - ((b - eff).astype(np.float32) / cur_sca).astype(np.float32)).astype(np.float32) * recip_thickness).astype(np.float32)
    aia = (((dzp * abs_lens_left).astype(np.float32) - ((b - eff).astype(np.float32) / cur_abs).astype(np.float32)).astype(np.float32) * recip_thickness).astype(np.float32)
    while True:
        # c.cl:643-668, the two loops side by side: a lane walks while it is not in its last layer and both sums keep their sign
        go = np.where(down, (j > 0) & (ais < 0) & (aia < 0), (j < n - 1) & (ais > 0) & (aia > 0))
        if not go.any():
            break
        j = np.where(go, np.where(down, j - 1, j + 1), j)
        b = np.where(go, np.where(down, b - thickness, b + thickness), b).astype(np.float32)
        new_sca, new_abs = lengths_in(j)
        cur_sca, cur_abs = np.where(go, new_sca, cur_sca), np.where(go, new_abs, cur_abs)
        r_sca, r_abs = (F(1) / cur_sca).astype(np.float32), (F(1) / cur_abs).astype(np.float32)
        ais = np.where(go, np.where(down, ais + r_sca, ais - r_sca), ais).astype(np.float32)
        aia = np.where(go, np.where(down, aia + r_abs, aia - r_abs), aia).astype(np.float32)
    same = (j == j0) | (np.abs(dzp) < EPSILON)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        recip_dz = (F(1) / dzp).astype(np.float32)
        far_sca = ((((((ais * thickness).astype(np.float32) * cur_sca).astype(np.float32) + b).astype(np.float32) - eff).astype(np.float32)) * recip_dz).astype(np.float32)
        far_abs = ((((((aia * thickness).astype(np.float32) * cur_abs).astype(np.float32) + b).astype(np.float32) - eff).astype(np.float32)) * recip_dz).astype(np.float32)
    distance = np.where(same, (sca_step_left * cur_sca).astype(np.float32), far_sca)
    to_absorption = np.where(same, (abs_lens_left * cur_abs).astype(np.float32), far_abs)

    def per_step(v):
        return np.ascontiguousarray(v.reshape(shape).T)
    return dict(start=per_step(j0), end=per_step(j), crossings=per_step(np.abs(j - j0)), absorbed=per_step((to_absorption < distance).astype(np.int64)), dz=dz)


# ---- the oracle's two bunches and the guard ----
N_BUNCHES = 2
MIN_LONG_TRIPS, MIN_END_WALKS, MIN_DETECTED = 200, 50, 50           # per bunch: trips across >= 5 layers, walks ending in layer 0 or the last, photons
_oracle = {}


def oracle_bunches(name):
    """[dict(records=sorted records as bytes, x=RNG words, count=hits, trips=first_trips(...))] for the two bunches on continuing
    streams: computed once per recipe, shared by its cases and by the CPU guard"""
    if name not in _oracle:
        R = recipe(name)
        x, a = R.streams
        out = []
        for _ in range(N_BUNCHES):
            ph, cnt, x_after, _ = capi.propagate(R.T, R.steps, x, a, threads=8)
            states = prefix_states(R.T, R.steps, x, a)
            # the restatement's random numbers are the oracle's: photon by photon the placed steps' streams end where the bunch leaves them
            assert np.array_equal(states[-1], x_after[:PLACED]), name
            trips = first_trips(R.T, R.med_o, R.steps, x, a, states)
            ph = capi.replace_indices_with_ids(ph, R.T.geo)
            out.append(dict(records=common.sort_photons(ph).tobytes(), x=x_after, count=cnt, trips=trips))
            x = x_after
        _oracle[name] = out
    return _oracle[name]


def guard(name):
    """the non-vacuity conditions, from the oracle alone: raises AssertionError, returns the figures per bunch"""
    R = recipe(name)
    n = int(R.med_o["num_layers"])
    what = np.array(R.placed_what)
    figures = []
    x, a = R.streams
    u, x_after = uniform_draws(x[:64], a[:64], 5)
    u_o, x_o = capi.sample(R.T, "uniform", x[:64], a[:64], 5)
    assert np.array_equal(u.T.view(np.uint32), u_o.view(np.uint32)) and np.array_equal(x_after, x_o), name
    for b, o in enumerate(oracle_bunches(name)):
        t = o["trips"]
        long_trips = int((t["crossings"] >= 5).sum())
        end_walks = int(((t["end"] == 0) | (t["end"] == n - 1)).sum())
        figures.append(dict(long_trips=long_trips, end_walks=end_walks, detected=o["count"], most=int(t["crossings"].max())))
        msg = "%s, bunch %d: %r" % (name, b, figures[-1])
        assert long_trips >= MIN_LONG_TRIPS and end_walks >= MIN_END_WALKS and o["count"] >= MIN_DETECTED, msg

        def of(prefix):
            sel = np.array([w.startswith(prefix) for w in what])
            assert sel.any(), prefix
            return {k: t[k][sel] for k in ("start", "end", "crossings", "absorbed")}, t["dz"][sel]
        # the last layer on entry: no step of the loop, both directions
        for prefix, layer in (("layer 0 heading down", 0), ("last layer heading up", n - 1)):
            v, _ = of(prefix)
            assert np.all(v["start"] == layer) and np.all(v["crossings"] == 0), msg
        # the last layer reached in mid-walk: from one layer away the first crossing ends the walk there, whatever the budgets say.  (From
        # two layers away the second crossing needs 10 m in one trip; the ends of SPICE-Mie's stack scatter every half metre, so those
        # walks stop one layer short there -- they are placed as the issue asks, and asserted to take the step they can.)
        for k in (1, 2):
            v, _ = of("%d from the bottom heading down" % k)
            assert np.all(v["start"] == k) and np.count_nonzero((v["end"] == k - 1) & (v["crossings"] == 1)) >= 10, msg
            assert k > 1 or np.count_nonzero(v["end"] == 0) >= 10, msg
            v, _ = of("%d from the top heading up" % k)
            assert np.all(v["start"] == n - 1 - k) and np.count_nonzero((v["end"] == n - k) & (v["crossings"] == 1)) >= 10, msg
            assert k > 1 or np.count_nonzero(v["end"] == n - 1) >= 10, msg
        # dz around zero: both signs below kEpsilon and above it, and nothing flat crosses a layer
        _, dz = of("dz around zero")
        assert np.any((dz > 0) & (dz < 1e-6)) and np.any((dz < 0) & (dz > -1e-6)), (msg, dz)
        assert np.any((dz > 4e-6) & (dz < EPSILON)) and np.any((dz < -4e-6) & (dz > -EPSILON)) and np.any(dz > 1.5e-5) and np.any(dz < -1.5e-5), (msg, dz)
        # on the boundaries, both directions (round 9's placement)
        v, dz = of("on layer boundary")
        assert np.any(dz < 0) and np.any(dz > 0) and len(dz) == 12, msg
        # the absorption budget ends inside the first crossed layer
        v, _ = of("just ")
        assert np.count_nonzero((v["crossings"] == 1) & (v["absorbed"] == 1)) >= 10, msg
        # long walks: within 1e-3 of +-z
        v, dz = of("near vertical")
        assert np.all(np.abs(dz) > 1.0 - 1e-6) and np.any(dz < 0) and np.any(dz > 0), msg
    return figures
