"""Inputs and checks shared by tests/test_propagation_reference.py (the oracle) and tests/test_propagation_reference_gpu.py (the
kernels): bunches of clear-ice rays and cascade bunches with photon histories, and the assertions that hold a set of photon records
to the float64 statements of tests/propagation_reference.py.  Every condition on the inputs (which rays are fragile, left out, how
many a class keeps) is computed from the statement alone, so it is the same on both sides.  A plain module: nothing runs on import."""
import math
import os

import numpy as np

from clsim_amd import synthetic as S
from oracle import builders as B
from oracle import capi
from tests import common
from tests import kernel_matrix as KM
from tests import propagation_reference as PR

N_RAYS = 16384
CLEAR_LENGTH = 1e7
FLASHER_WLEN = np.float32(common.FLASHER_WLEN)
CLASSES = ("near", "inside", "axis", "tangent", "vertical", "far")
# rays per class; the far class is small and mostly at 300 ... 400 m: beyond, E(r) approaches R^2 and most rays are fragile BY
# GEOMETRY (tests/propagation_reference.py (1)), and fragile rays are capped at 1 % of the bunch
CLASS_SIZES = dict(near=9408, inside=2048, axis=2048, tangent=2048, vertical=512, far=320)
FAR_TAIL = 64                     # of the far class: 400 ... 1500 m, log-uniform
MAX_FRAGILE, MAX_LEFT_OUT, MAX_FLAT, MIN_DECIDED = 0.01, 0.001, 0.001, 200
assert sum(CLASS_SIZES.values()) == N_RAYS


def geometry(name):
    if name == "ic86":
        return S.ic86_geometry()
    if name == "regular":
        return S.ic86_geometry(jitter=0.0)
    if name == "60":                       # common.config("<name>_60")'s detector: 52 standard strings and the 8 dense ones
        g = S.ic86_geometry()
        ids = np.asarray(g["string_ids"])
        keep = (ids <= 52) | (ids >= 79)
        return {k: (np.asarray(v)[keep] if (hasattr(v, "__len__") and not isinstance(v, str) and len(v) == len(ids)) else v) for k, v in g.items()}
    assert name == "large"
    return S.large_detector_geometry(side=12)          # 144 strings, 8 640 DOMs: the brute force stays within seconds


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _perpendicular(u):
    """two unit vectors that span the plane perpendicular to each u"""
    helper = np.where(np.abs(u[:, 2:3]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    e1 = np.cross(u, helper)
    e1 /= np.linalg.norm(e1, axis=1)[:, None]
    return e1, np.cross(u, e1)


def ray_steps(geom, seed):
    """N_RAYS flasher steps of ONE photon and length 0 -- the photon IS the ray (step position, step direction) -- and the class of
    each.  Sources sit near a random DOM and aim at a point within 1.3 R of its centre, so about half of them hit."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = N_RAYS
    c = np.stack([np.asarray(geom[k], dtype=np.float64) for k in ("x", "y", "z")], axis=1)
    sid = np.asarray(geom["string_ids"])
    R = float(geom["om_radius"])
    cls = np.repeat(np.arange(len(CLASSES)), [CLASS_SIZES[k] for k in CLASSES])
    rng.shuffle(cls)
    is_ = {k: cls == i for i, k in enumerate(CLASSES)}
    dom = rng.integers(0, len(c), size=n)
    u = _unit(rng, n)                                              # from the DOM towards the source
    far = np.exp(rng.uniform(math.log(400.0), math.log(1500.0), n))
    far_rank = np.cumsum(is_["far"])
    dist = np.select([is_["inside"], is_["far"] & (far_rank > FAR_TAIL), is_["far"]],
                     [R * rng.random(n) ** (1.0 / 3.0), rng.uniform(300.0, 400.0, n), far], default=rng.uniform(1.5, 30.0, n))
    src = c[dom] + u * dist[:, None]
    rho, ang = 1.3 * R * np.sqrt(rng.random(n)), rng.uniform(0.0, 2.0 * np.pi, n)
    e1, e2 = _perpendicular(u)
    aim = c[dom] + rho[:, None] * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
    # on the string axis (the mean x, y of its DOMs), between this DOM and the next one of the string, aimed at either
    nxt = np.minimum(dom + 1, len(c) - 1)
    nxt = np.where(sid[nxt] == sid[dom], nxt, dom - 1)
    axis_xy = {s: (c[sid == s, 0].mean(), c[sid == s, 1].mean()) for s in np.unique(sid)}
    ax = np.array([axis_xy[s] for s in sid[dom]])
    frac = rng.uniform(0.2, 0.8, n)
    on_axis = np.stack([ax[:, 0], ax[:, 1], c[dom, 2] + frac * (c[nxt, 2] - c[dom, 2])], axis=1)
    target = np.where(rng.random(n) < 0.5, dom, nxt)
    aim_axis = c[target] + np.stack([rho * np.cos(ang), rho * np.sin(ang), np.zeros(n)], axis=1)
    src = np.where(is_["axis"][:, None], on_axis, src)
    aim = np.where(is_["axis"][:, None], aim_axis, aim)
    # tangent: the DOM's centre exactly beside the source (urdot = 0 to a millimetre), at every impact parameter up to 1.3 R
    d_t = _unit(rng, n)
    t1, t2 = _perpendicular(d_t)
    beside = c[dom] + rho[:, None] * (np.cos(ang)[:, None] * t1 + np.sin(ang)[:, None] * t2) + rng.normal(0.0, 1e-3, n)[:, None] * d_t
    src = np.where(is_["tangent"][:, None], beside, src)
    aim = np.where(is_["tangent"][:, None], beside + d_t, aim)
    # vertical: below a DOM, within 1.3 R of its x, y, going straight up (theta = 0 exactly: dirLenXYSqr = 0)
    below = c[dom] + np.stack([rho * np.cos(ang), rho * np.sin(ang), -dist], axis=1)
    src = np.where(is_["vertical"][:, None], below, src)
    d = aim - src
    d /= np.linalg.norm(d, axis=1)[:, None]
    st = np.zeros(n, dtype=capi.STEP_DTYPE)
    st["x"], st["y"], st["z"] = src[:, 0], src[:, 1], src[:, 2]
    st["t"] = rng.uniform(0.0, 1000.0, n)
    st["theta"] = np.where(is_["vertical"], 0.0, np.arccos(np.clip(d[:, 2], -1.0, 1.0)))
    st["phi"] = np.arctan2(d[:, 1], d[:, 0]) % (2.0 * np.pi)
    st["length"], st["beta"], st["num"], st["sourceType"] = 0.0, 1.0, 1, 1
    st["weight"] = rng.uniform(0.5, 2.0, n)
    st["id"] = np.arange(n, dtype=np.uint32)
    return st, cls


def first_uniforms(x, a, k=4):
    return np.array([capi.eval_rng(int(x[i]), int(a[i]), k)[0] for i in range(len(x))], dtype=np.float64)


_ray_cases = {}


def ray_case(geom_name, pancake, seed=5):
    """the bunch, its streams and the float64 statement's verdict on every ray; made once and left unchanged"""
    key = (geom_name, pancake, seed)
    if key in _ray_cases:
        return _ray_cases[key]
    geom = geometry(geom_name)
    steps, cls = ray_steps(geom, seed)
    x, a = common.streams(N_RAYS)
    p = np.stack([steps[k].astype(np.float64) for k in ("x", "y", "z")], axis=1)
    d = PR.ray_directions(steps["theta"], steps["phi"])
    st = PR.first_dom(geom, p, d, pancake=pancake)
    # draws: a photon whose first free paths are short scatters or dies before the DOM -- resp., where the statement sees no
    # DOM, before it has left the detector (the sphere around the origin that holds every DOM)
    c = np.stack([np.asarray(geom[k], dtype=np.float64) for k in ("x", "y", "z")], axis=1)
    radius = np.linalg.norm(c, axis=1).max() + st["R"]
    pd = np.einsum("ij,ij->i", p, d)
    leave = np.maximum(-pd + np.sqrt(np.maximum(pd * pd - np.einsum("ij,ij->i", p, p) + radius * radius, 0.0)), 0.0)
    horizon = np.where(st["hit"], st["s"], leave)
    un = first_uniforms(x, a)
    with np.errstate(divide="ignore"):
        free = np.minimum(-np.log(un), -np.log(1.0 - un)).min(axis=1) * CLEAR_LENGTH
    left_out = free < 1.01 * horizon
    case = dict(geom=geom, geom_name=geom_name, pancake=pancake, steps=steps, cls=cls, streams=(x, a), p=p, d=d, st=st, left_out=left_out,
                decided=~st["fragile"] & ~left_out)
    _ray_cases[key] = case
    return case


def clear_medium_o():
    return B.homogeneous_medium(abs_len=CLEAR_LENGTH, sca_len=CLEAR_LENGTH)


def oracle_tables_for(geom, med_o, flasher, pancake, stop_detected=True, history_entries=0):
    geo = B.build_geometry(geom["string_ids"], geom["dom_ids"], geom["x"], geom["y"], geom["z"], geom["subdetectors"], geom["om_radius"])
    bias = B.icecube_dom_acceptance()
    gens = [B.cherenkov_wlen_generator(bias, med_o)] + ([dict(kind="const", value=common.FLASHER_WLEN)] if flasher else [])
    return capi.make_tables(med_o, geo, gens, bias, pancake=pancake, stop_detected=stop_detected, history_entries=history_entries)


def oracle_rays(case, stop_detected=True, build_geometry=None):
    """the oracle's records of the bunch, string and DOM fields as IDs"""
    T = oracle_tables_for(case["geom"], clear_medium_o(), True, case["pancake"], stop_detected)
    x, a = case["streams"]
    ph, cnt, _, _ = capi.propagate(T, case["steps"], x, a, threads=8, max_hits=8 * N_RAYS)
    assert cnt == len(ph)
    return capi.replace_indices_with_ids(ph, T.geo)


def caps_message(case):
    st, cls = case["st"], case["cls"]
    per_class = ", ".join("%s %d/%d" % (k, int((case["decided"] & (cls == i)).sum()), int((cls == i).sum())) for i, k in enumerate(CLASSES))
    return ("fragile %.3f %%, left out by draws %.3f %%, start inside %.2f %%, predicted hits %d; decided per class: %s"
            % (100.0 * st["fragile"].mean(), 100.0 * case["left_out"].mean(), 100.0 * st["inside"].mean(), int(st["hit"].sum()), per_class))


def check_ray_caps(case):
    msg = caps_message(case)
    assert case["st"]["fragile"].mean() <= MAX_FRAGILE, msg
    assert case["left_out"].mean() <= MAX_LEFT_OUT, msg
    for i, k in enumerate(CLASSES):
        assert int((case["decided"] & (case["cls"] == i)).sum()) >= MIN_DECIDED, msg
    v = case["cls"] == CLASSES.index("vertical")
    assert case["st"]["vertical"][v].all() and not case["st"]["hit"][v].any(), msg


def _ids_of(geom, dom):
    return np.asarray(geom["string_ids"])[dom], np.asarray(geom["dom_ids"])[dom]


def check_rays(case, ph, what):
    """stop mode: the records `ph` of the bunch against statement (a) on every decided ray.  Returns {quantity: worst error / bound}."""
    check_ray_caps(case)
    st, steps, decided, geom, pancake = case["st"], case["steps"], case["decided"], case["geom"], case["pancake"]
    msg = what + ": " + caps_message(case)
    n = N_RAYS
    ray = ph["id"].astype(np.int64)
    assert len(np.unique(ray)) == len(ray), msg + "; a ray with two records"
    got = np.zeros(n, bool)
    got[ray] = True
    wrong = decided & (got != st["hit"])
    assert not wrong.any(), "%s; %d decided rays detected against the statement, first: ray %d (class %s) detected %s, statement s = %r, disc = %r" % (
        msg, int(wrong.sum()), int(np.flatnonzero(wrong)[0]), CLASSES[case["cls"][np.flatnonzero(wrong)[0]]], bool(got[np.flatnonzero(wrong)[0]]),
        st["s"][np.flatnonzero(wrong)[0]], st["disc"][np.flatnonzero(wrong)[0]])
    # undecided rays: reported, never asserted on
    keep = decided[ray] & st["hit"][ray]
    r, i = ph[keep], ray[keep]
    want_string, want_dom = _ids_of(geom, st["dom"][i])
    same = (r["stringID"] == want_string) & (r["omID"] == want_dom)
    assert same.all(), "%s; %d of %d decided hits on another DOM than the statement's" % (msg, int((~same).sum()), len(r))
    return _check_records(case["p"][i], case["d"][i], steps[i], st["dom"][i], r, geom, pancake, msg, s=st["s"][i], ds=st["delta_s"][i], scattered=False)


def _check_records(q, d, steps, dom, r, geom, pancake, msg, s, ds, scattered):
    """the fields of records r that hit DOM `dom` coming from q along d after s metres on that last stretch"""
    c = np.stack([np.asarray(geom[k], dtype=np.float64) for k in ("x", "y", "z")], axis=1)[dom]
    R, delta_c = float(geom["om_radius"]), PR.dom_position_error(geom)
    worst = {}

    def hold(name, err, bound):
        bound = PR.SAFETY * np.asarray(bound, dtype=np.float64)
        ratio = np.asarray(err, dtype=np.float64) / bound
        worst[name] = float(ratio.max()) if len(ratio) else 0.0
        k = int(np.argmax(ratio)) if len(ratio) else 0
        assert worst[name] <= 1.0, "%s; %s: worst error %.3g against its bound %.3g (record %d)" % (msg, name, np.ravel(err)[k], np.ravel(bound)[k], k)

    wl = r["wavelength"].astype(np.float64)
    M = np.maximum(np.abs(q).max(axis=1), np.abs(q + s[:, None] * d).max(axis=1))
    pos = np.stack([r[k].astype(np.float64) for k in ("x", "y", "z")], axis=1)
    d_pos = ds + delta_c + 4.0 * PR.ulp32(M)
    hold("position", np.abs(pos - PR.expected_hit_position(c, q, d, s, pancake)).max(axis=1), d_pos)
    hold("radius", np.abs(np.linalg.norm(pos, axis=1) - R / pancake), d_pos)
    if not scattered:
        v = PR.group_velocity(dict(n=B.REFINDEX_N, g=B.REFINDEX_G), wl)
        hold("cherenkovDist", np.abs(r["cherenkovDist"] - s), ds + 2.0 * PR.ulp32(s))
        t = steps["t"].astype(np.float64) + s / v
        hold("time", np.abs(r["t"] - t), ds / v + 2.0 * PR.ulp32(t))
        d_theta, d_phi = PR.angle_bounds(steps["theta"])
        hold("theta", np.abs(r["theta"] - steps["theta"].astype(np.float64)), d_theta)
        dphi = np.abs(r["phi"] - steps["phi"].astype(np.float64))
        hold("phi", np.minimum(dphi, 2.0 * np.pi - dphi), d_phi)
        hold("groupVelocity", np.abs(r["groupVelocity"] / v - 1.0), np.full(len(r), 8.0 * PR.U))
        assert np.all(r["numScatters"] == 0) and np.all(r["wavelength"] == FLASHER_WLEN), msg
        for a_, b_ in (("sx", "x"), ("sy", "y"), ("sz", "z"), ("st", "t")):
            assert np.array_equal(r[a_], steps[b_]), msg + "; start " + b_
    bias = B.icecube_dom_acceptance()                 # (the table's DATA; its interpolation is PR's)
    w = steps["weight"].astype(np.float64) / PR.wavelength_bias(bias, wl)
    hold("weight", np.abs(r["weight"] / w - 1.0), PR.weight_bound(bias, wl))
    return worst


def check_rays_kept(case, ph, what):
    """without STOP_PHOTONS_ON_DETECTION: every record is a true intersection of its ray (soundness), and a decided ray with exactly one
    DOM on its way gives exactly that record.  Which of several DOMs the reference keeps is its bit masks' business (oracle/
    clsim_oracle.c: checkForCollision_OnString_keep) and stays with the oracle."""
    check_ray_caps(case)
    st, steps, geom, pancake = case["st"], case["steps"], case["geom"], case["pancake"]
    msg = what + ": " + caps_message(case)
    first = ph[ph["numScatters"] == 0]                 # (a photon that scattered 1e7 m away never comes back; be explicit)
    ray = first["id"].astype(np.int64)
    index = {(int(s_), int(d_)): k for k, (s_, d_) in enumerate(zip(geom["string_ids"], geom["dom_ids"]))}
    dom = np.array([index[(int(s_), int(d_))] for s_, d_ in zip(first["stringID"], first["omID"])], dtype=np.int64)
    c = np.stack([np.asarray(geom[k], dtype=np.float64) for k in ("x", "y", "z")], axis=1)
    b, disc, s, E, ds = PR.intersection(c[dom], st["R"], st["delta_c"], case["p"][ray], case["d"][ray], pancake)
    sound = (disc >= -E) & (s >= -ds) & ~st["vertical"][ray]
    assert sound.all(), "%s; %d records that are no intersection of their ray" % (msg, int((~sound).sum()))
    clear = disc >= E
    worst = _check_records(case["p"][ray][clear], case["d"][ray][clear], steps[ray][clear], dom[clear], first[clear], geom, pancake, msg,
                           s=s[clear], ds=ds[clear], scattered=False)
    # exactly one DOM on the way, and that DOM out of the reach of the reference's shared mask bits (PR.never_masked)
    single = case["decided"] & (st["n_candidates"] == 1)
    one = single & PR.never_masked(geom)[np.maximum(st["dom"], 0)]
    per_ray = np.bincount(ray, minlength=N_RAYS)
    assert one.sum() >= 1000 and np.all(per_ray[one] == 1) and np.all(per_ray[single] <= 1), (
        "%s; %d rays with one DOM on their way, %d of them beyond the masks, %d of those without exactly one record" % (
            msg, int(single.sum()), int(one.sum()), int((per_ray[one] != 1).sum())))
    sel = single[ray]
    assert np.array_equal(dom[sel], st["dom"][ray[sel]]), msg
    worst["rays with one DOM, masked by the reference"] = int((single & ~one & (per_ray == 0)).sum())
    none = case["decided"] & (st["n_candidates"] == 0)
    assert np.all(per_ray[none] == 0), msg
    worst["rays with one DOM"] = int(one.sum())
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer walk from photon histories
# ---------------------------------------------------------------------------------------------------------------------------------

WALK_MEDIA = ("mie", "lea", "photonics_mie", "constant_tilt_aniso")
WALK_STEPS, WALK_PHOTONS, WALK_PANCAKE = 512, 200, 5.0
HISTORY = 64                      # the most the oracle keeps (ORACLE_MAX_HISTORY); the share of complete paths is asserted


def walk_medium_o(name):
    if name in ("mie", "lea"):
        return B.load_ppc_ice(os.path.join(common.ICE, "spice_" + name))
    if name == "photonics_mie":
        return B.load_photonics_ice(common.PHOTONICS[name])
    assert name == "constant_tilt_aniso"               # tests/kernel_matrix.py: media(("constant", True, True, ...)), its oracle side
    lea = B.load_ppc_ice(os.path.join(common.ICE, "spice_lea"))
    abs_len, sca_len = KM.constant_lengths(lea)
    med = {k: v for k, v in lea.items() if k not in ("alpha", "kappa", "A", "B", "D", "E", "aDust400", "deltaTau", "b400")}
    med.update(len_mode="constant", abs_const=abs_len, sca_const=sca_len)
    return med


def walk_steps(name):
    steps = S.cascade_steps(WALK_STEPS, seed=41 + WALK_MEDIA.index(name), photons_per_step=WALK_PHOTONS)
    steps["t"] = np.linspace(0.0, 500.0, len(steps))
    return steps


def oracle_walk(name):
    """(records with IDs, histories oldest first)"""
    geom = geometry("ic86")
    T = oracle_tables_for(geom, walk_medium_o(name), False, WALK_PANCAKE, history_entries=HISTORY)
    steps = walk_steps(name)
    x, a = common.streams(len(steps))
    ph, cnt, _, _, raw = capi.propagate(T, steps, x, a, history=True)
    assert cnt == len(ph)
    return capi.replace_indices_with_ids(ph, T.geo), capi.convert_photon_histories(raw, ph, HISTORY)


def check_walk(name, ph, hist, what, statement=PR.absorption_lengths_used):
    """every record and its history against statement (c) and the invariants of a record.  Returns {quantity: worst error / bound}."""
    medium = walk_medium_o(name)
    geom = geometry("ic86")
    pancake = WALK_PANCAKE
    n = len(ph)
    assert n >= KM.MIN_HITS, "%s: %d photons detected" % (what, n)
    ns = ph["numScatters"].astype(np.int64)
    complete = ns <= HISTORY
    used_records = (ns >= 1) & complete
    index = {(int(s_), int(d_)): k for k, (s_, d_) in enumerate(zip(geom["string_ids"], geom["dom_ids"]))}
    dom = np.array([index[(int(s_), int(d_))] for s_, d_ in zip(ph["stringID"], ph["omID"])], dtype=np.int64)
    c = np.stack([np.asarray(geom[k], dtype=np.float64) for k in ("x", "y", "z")], axis=1)
    start = np.stack([ph[k].astype(np.float64) for k in ("sx", "sy", "sz")], axis=1)
    last = np.array([hist[i][-1, :3].astype(np.float64) if len(hist[i]) else start[i] for i in range(n)])
    a_last = np.array([float(hist[i][-1, 3]) if len(hist[i]) else 0.0 for i in range(n)])
    d = PR.ray_directions(ph["theta"], ph["phi"])
    R, delta_c = float(geom["om_radius"]), PR.dom_position_error(geom)
    b, disc, s, E, ds = PR.intersection(c[dom], R, delta_c, last, d, pancake)
    msg = "%s: %d records, %.1f %% with their whole path, %d scattered ones used" % (what, n, 100.0 * complete.mean(), int(used_records.sum()))
    assert complete.mean() >= 0.5, msg
    assert np.all(disc >= -E) and np.all(s >= -ds), msg + "; a record that is no intersection of its last stretch"
    clear = disc >= E
    steps = np.zeros(n, dtype=capi.STEP_DTYPE)
    steps["weight"] = 1.0
    worst = _check_records(last[clear], d[clear], steps[clear], dom[clear], ph[clear], geom, pancake, msg, s=s[clear], ds=ds[clear], scattered=True)

    def hold(name_, err, bound, k=None):
        bound = PR.SAFETY * bound
        ratio = float(err) / float(bound)
        if ratio > worst.get(name_, (0.0,))[0]:
            worst[name_] = (ratio, float(err), float(bound), k)

    wl = ph["wavelength"].astype(np.float64)
    v = PR.group_velocity(medium, wl)
    gv = np.abs(ph["groupVelocity"] / v - 1.0)
    assert gv.max() <= PR.SAFETY * 8.0 * PR.U, "%s; groupVelocity: worst relative error %.3g against %g u" % (msg, gv.max(), 8.0 * PR.SAFETY)
    worst["groupVelocity"] = float(gv.max() / (PR.SAFETY * 8.0 * PR.U))
    # t - st = cherenkovDist / groupVelocity, both accumulated per trip in float32: one rounding of each per trip
    t_err = np.abs((ph["t"].astype(np.float64) - ph["st"]) - ph["cherenkovDist"].astype(np.float64) / ph["groupVelocity"])
    t_bound = PR.SAFETY * (ns + 2) * (PR.ulp32(ph["t"]) + PR.ulp32(ph["cherenkovDist"]) / v)
    assert np.all(t_err <= t_bound), "%s; time of flight: worst error / bound %.3g" % (msg, (t_err / t_bound).max())
    worst["time of flight"] = float((t_err / t_bound).max())
    segments = flat_segments = 0
    for i in range(n):
        lengths = PR.absorption_lengths_of_layers(medium, wl[i])
        pts = np.concatenate([start[i][None, :], hist[i][:, :3].astype(np.float64)]) if complete[i] else hist[i][:, :3].astype(np.float64)
        a_pts = np.concatenate([[0.0], hist[i][:, 3].astype(np.float64)]) if complete[i] else hist[i][:, 3].astype(np.float64)
        path = 0.0
        for j in range(len(pts) - 1):
            used, bound, flat, _ = statement(medium, pts[j], pts[j + 1], wl[i], lengths=lengths)
            path += float(np.linalg.norm(pts[j + 1] - pts[j]))
            segments += 1
            if flat:
                flat_segments += 1
                continue
            hold("segment", abs((a_pts[j + 1] - a_pts[j]) - used), bound, (i, j))
        if not clear[i]:
            continue
        # the last stretch: distInAbsLens is taken at the would-be scatter point, beyond the DOM (oracle/clsim_oracle.c:1063-1073)
        used, bound, flat, _ = statement(medium, last[i], last[i] + s[i] * d[i], wl[i], lengths=lengths)
        if not flat:
            hold("last stretch", max(used - (float(ph["distInAbsLens"][i]) - a_last[i]), 0.0), bound + ds[i] / lengths.min(), (i, -1))
        if complete[i]:
            # cherenkovDist is the polyline's length: a float32 sum of ns + 1 float32 distances between float32 points
            hold("path length", abs(float(ph["cherenkovDist"][i]) - (path + s[i])),
                 ds[i] + (ns[i] + 1) * (PR.ulp32(ph["cherenkovDist"][i]) + 2.0 * PR.ulp32(np.abs(pts).max())), (i, -1))
    msg += "; %d segments, %d left out as flat" % (segments, flat_segments)
    assert segments >= 200 and flat_segments <= MAX_FLAT * segments, msg
    for name_ in ("segment", "last stretch", "path length"):
        ratio, err, bound, k = worst.get(name_, (0.0, 0.0, 1.0, None))
        assert ratio <= 1.0, "%s; %s: worst error %.3g against its bound %.3g (record, segment %r)" % (msg, name_, err, bound, k)
        worst[name_] = ratio
        worst[name_ + " (absolute)"] = err
    worst["segments"], worst["complete"] = segments, float(complete.mean())
    return worst
