"""Muon slicer (clsimhip_slice_muons) against the independent float64 Python statement in tests/muon_slicer_reference.py: bit for bit
on every output field and on the relabel table, path by path of the reference's I3MuonSlicer; every refusal, asserted not to write;
properties on 200 random trees."""
import math
import random
import struct

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import muon_slicer_reference as R

C = R.C
FIELDS = ("type", "shape", "x", "y", "z", "time", "dx", "dy", "dz", "energy", "length", "identifier")
FIRST = 1000


def node(identifier, parent, type=CV.ParticleType.EMinus, x=0.0, y=0.0, z=0.0, time=0.0, direction=(0.0, 0.0, 1.0), energy=1.0, length=math.nan,
         speed=C, shape=0, flags=0):
    return dict(type=type, shape=shape, x=x, y=y, z=z, time=time, dx=direction[0], dy=direction[1], dz=direction[2], energy=energy, length=length,
                identifier=identifier, speed=speed, parent=parent, flags=flags)


def muon(identifier, parent, length, energy=100.0, **kw):
    return node(identifier, parent, type=CV.ParticleType.MuMinus, length=length, energy=energy, **kw)


def on_track(mu, identifier, parent, s, energy, off=0.0, dt=0.0, **kw):
    """a daughter at distance s along the muon's track, `off` metres beside it (the tracks here run along z or x), at the track's time + dt"""
    d = (mu["dx"], mu["dy"], mu["dz"])
    side = (0.0, 1.0, 0.0)
    return node(identifier, parent, x=mu["x"] + s * d[0] + off * side[0], y=mu["y"] + s * d[1] + off * side[1], z=mu["z"] + s * d[2] + off * side[2],
                time=mu["time"] + s / mu["speed"] + dt, energy=energy, **kw)


def track(mu, Ei=None, Ef=0.0, ti=None, tf=None):
    ti = mu["time"] if ti is None else ti
    return dict(identifier=mu["identifier"], Ei=mu["energy"] if Ei is None else Ei, Ef=Ef, ti=ti, tf=mu["time"] + mu["length"] / mu["speed"] if tf is None else tf)


def to_arrays(tree, tracks):
    t = np.zeros(len(tree), dtype=CV.TREE_PARTICLE_DTYPE)
    for i, n in enumerate(tree):
        for f in FIELDS:
            t["particle"][f][i] = n[f]
        t["speed"][i], t["parent"][i], t["flags"][i] = n["speed"], n["parent"], n["flags"]
    k = np.zeros(len(tracks), dtype=CV.MMC_TRACK_DTYPE)
    for i, n in enumerate(tracks):
        for f in ("identifier", "Ei", "Ef", "ti", "tf"):
            k[f][i] = n[f]
    return t, k


def bits(v):
    return struct.pack("<d", v)


def check(tree, tracks, first=FIRST):
    """runs both and holds them to each other bit for bit; returns the reference's result"""
    want, want_relabel, want_counters = R.slice_muons(tree, tracks, first)
    got, relabel, counters = CV.slice_muons(*to_arrays(tree, tracks), first)
    assert counters == want_counters
    assert [(int(a), int(b)) for a, b in relabel] == want_relabel
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for f in FIELDS:
            if isinstance(w[f], float):
                assert bits(float(g["particle"][f])) == bits(w[f]), (f, g, w)
            else:
                assert int(g["particle"][f]) == w[f], (f, g, w)
        assert bits(float(g["speed"])) == bits(w["speed"]) and int(g["parent"]) == w["parent"] and int(g["flags"]) == w["flags"], (g, w)
        assert int(g["particle"]["reserved"]) == 0
    return want, want_relabel, want_counters


def slices_of(out, relabel):
    ids = {a for a, _ in relabel}
    return [n for n in out if n["identifier"] in ids]


def with_daughters(n, energy=100.0, losses=1.0, length=50.0, **kw):
    mu = muon(1, -1, length, energy=energy, x=3.0, y=-2.0, z=10.0, time=100.0, **kw)
    step = length / (n + 1) if n else 0.0
    return [mu] + [on_track(mu, 2 + k, 0, step * (k + 1), losses) for k in range(n)], mu


@pytest.mark.parametrize("n", (0, 1, 3, 40))
def test_a_muon_with_daughters(n):
    tree, mu = with_daughters(n)
    out, relabel, counters = check(tree, [track(mu, Ef=20.0)])
    assert len(relabel) == n + 1 and len(out) == 2 * n + 2 and out[0]["flags"] == R.DARK
    assert all(s["flags"] == 0 and s["type"] == mu["type"] and s["parent"] == 0 for s in slices_of(out, relabel))
    assert [n_["identifier"] for n_ in out[1:]] == [x for k in range(n) for x in (FIRST + k, 2 + k)] + [FIRST + n]
    assert not any(counters.values())


def test_a_muon_that_is_not_in_the_track_list_and_invalid_energies():
    tree, mu = with_daughters(3)
    other = dict(track(mu), identifier=77)
    a, ra, _ = check(tree, [other])                                     # the particle's own energy and time, Ef = 0
    assert len(ra) == 4
    for bad in (dict(Ei=math.nan), dict(Ei=0.0), dict(Ei=-1.0), dict(Ef=math.nan), dict(Ef=-0.5), dict(Ei=math.nan, Ef=math.nan)):
        out, relabel, _ = check(tree, [dict(track(mu, Ef=5.0, ti=90.0), **bad)])
        assert len(relabel) == 4
    # without daughters, both invalid: an outgoing muon behind the can -- darkened, no slice (:421-429); one invalid: one slice
    lone, mu = with_daughters(0)
    out, relabel, _ = check(lone, [])
    assert len(out) == 1 and out[0]["flags"] == R.DARK and not relabel
    out, relabel, _ = check(lone, [track(mu, Ef=math.nan)])
    assert len(relabel) == 1


def test_stops_before_it_starts_and_zero_duration_only_darken():
    tree, mu = with_daughters(2)
    for tf, name in ((99.0, "stops_before_start"), (100.0, "zero_duration")):
        out, relabel, counters = check(tree, [track(mu, tf=tf)])
        assert not relabel and len(out) == 3 and out[0]["flags"] == R.DARK and counters[name] == 1 and sum(counters.values()) == 1


def test_both_sides_of_the_loss_rate_bound():
    tree, mu = with_daughters(3, energy=1000.0, losses=5.0)
    below = check(tree, [track(mu, Ef=990.0)])[0]                       # dEdt_calc = -5 / T, far below the bound
    above = check(tree, [track(mu, Ef=100.0)])[0]                       # dEdt_calc = 885 / T: the bound decides
    T = 50.0 / C
    Ei = 1000.0
    dEdt_max = (0.21 + 8.8e-3 * math.log(Ei) / R.LOG10) * C
    assert (990.0 - Ei + 15.0) / (0.0 - T) < dEdt_max < (100.0 - Ei + 15.0) / (0.0 - T)
    assert [s["energy"] for s in below if s["identifier"] >= FIRST] != [s["energy"] for s in above if s["identifier"] >= FIRST]


def test_losses_beyond_the_muons_energy():
    tree, mu = with_daughters(4, energy=10.0, losses=9.0)               # mid-track: the reset, then the early return behind the loop
    out, relabel, counters = check(tree, [track(mu)])
    assert counters["energy_reset"] == 1 and len(relabel) == 4 and out[-1]["identifier"] == 5
    assert [s["energy"] for s in slices_of(out, relabel)][3] == 0.0
    tree, mu = with_daughters(2, energy=10.0, losses=6.0)               # at the end only: no reset, no last slice
    out, relabel, counters = check(tree, [track(mu)])
    assert counters["energy_reset"] == 0 and len(relabel) == 2 and out[-1]["identifier"] == 3


def test_daughters_beside_the_track():
    mu = muon(1, -1, 50.0, time=5.0)
    near, far = on_track(mu, 2, 0, 10.0, 1.0, off=0.9e-3), on_track(mu, 3, 0, 20.0, 1.0, off=1.1e-3)
    child_of_far = node(4, 2, energy=0.5)
    out, relabel, counters = check([mu, near, far, child_of_far], [track(mu)])
    assert counters["off_track"] == 1
    assert [n["identifier"] for n in out] == [1, FIRST, 2, 3, FIRST + 1]                 # appended, not recursed into, the muon not split there


def test_a_daughter_with_a_nan_time_is_dropped():
    mu = muon(1, -1, 50.0)
    a, b = on_track(mu, 2, 0, 10.0, 1.0), on_track(mu, 3, 0, 20.0, 1.0)
    b["time"] = math.nan
    out, relabel, _ = check([mu, a, b, node(4, 2)], [track(mu)])
    assert [n["identifier"] for n in out] == [1, FIRST, 2, FIRST + 1]


def test_two_daughters_at_one_point_and_the_shortest_slices():
    mu = muon(1, -1, 50.0)
    out, relabel, _ = check([mu, on_track(mu, 2, 0, 10.0, 1.0), on_track(mu, 3, 0, 10.0, 1.0)], [track(mu)])
    assert [n["identifier"] for n in out] == [1, FIRST, 2, 3, FIRST + 1]
    for gap, emitted in ((0.09e-3, False), (0.11e-3, True)):
        out, relabel, _ = check([mu, on_track(mu, 2, 0, 10.0, 1.0), on_track(mu, 3, 0, 10.0 + gap, 1.0)], [track(mu)])
        assert (len(relabel) == 3) == emitted
        assert all(s["length"] >= 0.1e-3 for s in slices_of(out, relabel))
    # ... and behind the last daughter
    for gap, emitted in ((0.09e-3, False), (0.11e-3, True)):
        out, relabel, _ = check([mu, on_track(mu, 2, 0, 50.0 - gap, 1.0)], [track(mu)])
        assert (len(relabel) == 2) == emitted


def test_subtrees_primaries_and_a_long_slice():
    mu = muon(1, 0, 30.0, direction=(1.0, 0.0, 0.0), time=7.0)
    nu = node(9, -1, type=14, energy=1e3)                               # a non-muon primary above the muon
    first = on_track(mu, 2, 1, 10.0, 3.0)
    inner = muon(5, 2, 4.0, energy=2.0, x=first["x"], time=first["time"], direction=(0.0, 1.0, 0.0))     # a daughter's child: a muon with losses
    inner_loss = on_track(inner, 6, 3, 2.0, 0.5)
    inner_loss["x"], inner_loss["y"] = inner["x"], inner["y"] + 2.0
    plain = node(7, 2, energy=0.1)
    second = on_track(mu, 3, 1, 20.0, 3.0)
    other = muon(20, -1, 2500.0, energy=5e3, z=-500.0)                  # a second primary, one slice of 2.5 km
    tree = [nu, mu, first, inner, inner_loss, plain, second, other]
    out, relabel, counters = check(tree, [track(mu), track(inner), track(other)])
    assert [n["identifier"] for n in out] == [9, 1, FIRST, 2, 5, FIRST + 1, 6, FIRST + 2, 7, FIRST + 3, 3, FIRST + 4, 20, FIRST + 5]
    assert relabel == [(FIRST, 1), (FIRST + 1, 5), (FIRST + 2, 5), (FIRST + 3, 1), (FIRST + 4, 1), (FIRST + 5, 20)]
    assert counters["long_slice"] == 1
    assert [n["parent"] for n in out] == [-1, 0, 1, 1, 3, 4, 4, 4, 3, 1, 1, 1, -1, 12]
    # a muon without a length is copied and recursed into
    bare = muon(1, -1, math.nan)
    out, relabel, _ = check([bare, muon(2, 0, 10.0), node(3, 1, z=5.0, time=5.0 / C)], [])
    assert [n["identifier"] for n in out] == [1, 2, FIRST, 3, FIRST + 1] and out[0]["flags"] == 0 and out[1]["flags"] == R.DARK


def refusals():
    tree, mu = with_daughters(2)
    t = [track(mu)]
    yield "a muon below a muon", tree[:2] + [dict(tree[2], type=CV.ParticleType.MuPlus)], t, FIRST
    yield "type 0 below a muon", tree[:2] + [dict(tree[2], type=0)], t, FIRST
    for f in ("speed", "energy", "time"):
        yield "NaN " + f, [dict(mu, **{f: math.nan})] + tree[1:], t, FIRST
    yield "descending daughters", [tree[0], tree[2], tree[1]], t, FIRST
    yield "first daughter NaN", [tree[0], dict(tree[1], time=math.nan), tree[2]], t, FIRST
    yield "no energy but daughters", [dict(mu, energy=0.0)] + tree[1:], [], FIRST
    yield "track twice", tree, t + t, FIRST
    yield "parent >= index", [tree[0], dict(tree[1], parent=1), tree[2]], t, FIRST
    yield "parent < -1", [dict(tree[0], parent=-2)] + tree[1:], t, FIRST
    yield "slice identifier in use", tree, t, 1
    yield "slice identifier in use (last)", tree, t, 0
    yield "wrap", tree, t, 0xFFFFFFFE


@pytest.mark.parametrize("name,tree,tracks,first", list(refusals()), ids=[r[0] for r in refusals()])
def test_refusals_write_nothing(name, tree, tracks, first):
    with pytest.raises(R.Refused):
        R.slice_muons(tree, tracks, first)
    t, k = to_arrays(tree, tracks)
    out, relabel = np.full(16, 0xAB, dtype=np.uint8).view(np.uint8).repeat(104).view(CV.TREE_PARTICLE_DTYPE), np.full(16 * 8, 0xAB, dtype=np.uint8).view(CV.RELABEL_DTYPE)
    before = out.tobytes(), relabel.tobytes()
    import ctypes
    n_out, n_relabel, counters = ctypes.c_size_t(123), ctypes.c_size_t(456), np.full(5, 7, dtype=np.uint64)
    vp = ctypes.c_void_p
    rc = _lib.load().clsimhip_slice_muons(t.ctypes.data_as(vp), len(t), k.ctypes.data_as(vp), len(k), first, out.ctypes.data_as(vp), len(out), ctypes.byref(n_out),
                                          relabel.ctypes.data_as(vp), len(relabel), ctypes.byref(n_relabel), counters.ctypes.data_as(vp))
    assert rc == _lib.ERR_ARGUMENT
    assert (out.tobytes(), relabel.tobytes()) == before and n_out.value == 123 and n_relabel.value == 456 and (counters == 7).all()


def test_sizes_are_what_is_needed_and_at_most_the_capacities_are_written():
    import ctypes
    tree, mu = with_daughters(3)
    t, k = to_arrays(tree, [track(mu)])
    whole, whole_relabel, _ = CV.slice_muons(t, k, FIRST)
    out, relabel = np.zeros(5, dtype=CV.TREE_PARTICLE_DTYPE), np.zeros(3, dtype=CV.RELABEL_DTYPE)
    n_out, n_relabel = ctypes.c_size_t(), ctypes.c_size_t()
    vp = ctypes.c_void_p
    assert _lib.load().clsimhip_slice_muons(t.ctypes.data_as(vp), len(t), k.ctypes.data_as(vp), len(k), FIRST, out.ctypes.data_as(vp), 4, ctypes.byref(n_out),
                                            relabel.ctypes.data_as(vp), 2, ctypes.byref(n_relabel), None) == 0
    assert (n_out.value, n_relabel.value) == (8, 4)
    assert out[:4].tobytes() == whole[:4].tobytes() and not out[4:].tobytes().strip(b"\0")
    assert relabel[:2].tobytes() == whole_relabel[:2].tobytes() and not relabel[2:].tobytes().strip(b"\0")


def random_tree(rng):
    tree, tracks, next_id = [], [], [1]

    def new_id():
        next_id[0] += 1
        return next_id[0]

    def grow(parent, depth, at, time):
        kind = rng.random()
        if kind < 0.85 and depth < 3:
            d = rng.choice(((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.6, 0.0, 0.8)))
            mu = muon(new_id(), parent, rng.choice((math.nan, 0.0, 5.0, 80.0, 300.0, 900.0)), energy=rng.choice((0.5, 30.0, 4000.0)), x=at[0], y=at[1], z=at[2], time=time,
                      direction=d, speed=rng.choice((C, 0.29)), flags=rng.choice((0, 2)))
            tree.append(mu)
            me = len(tree) - 1
            if rng.random() < 0.7 and mu["length"] == mu["length"] and mu["length"] > 0:
                tracks.append(track(mu, Ei=rng.choice((None, math.nan, 0.0)), Ef=rng.choice((0.0, 1.0, math.nan, -1.0)),
                                    tf=rng.choice((None, None, mu["time"], mu["time"] - 1.0))))
            sliced = mu["length"] == mu["length"] and mu["length"] > 0
            places = sorted(rng.uniform(0.0, (mu["length"] if sliced else 10.0) * 1.05) for _ in range(rng.choice((0, 1, 2, 5))))
            for s in places:
                if rng.random() < 0.15 and depth < 2 and not sliced:
                    grow(me, depth + 1, (mu["x"] + s * d[0], mu["y"] + s * d[1], mu["z"] + s * d[2]), mu["time"] + s / mu["speed"])
                    continue
                loss = on_track(mu, new_id(), me, s, rng.choice((0.01, 1.0, 40.0)), off=rng.choice((0.0, 0.0, 0.0, 0.5e-3, 2e-3)), dt=rng.choice((0.0, 0.0, 1e-9)))
                tree.append(loss)
                if rng.random() < 0.2 and depth < 2:
                    grow(len(tree) - 1, depth + 1, (loss["x"], loss["y"], loss["z"]), loss["time"])
        else:
            tree.append(node(new_id(), parent, x=at[0], y=at[1], z=at[2], time=time, energy=rng.uniform(0.1, 10.0)))
            if rng.random() < 0.5 and depth < 3:
                grow(len(tree) - 1, depth + 1, at, time)

    for _ in range(rng.choice((1, 2, 3))):
        grow(-1, 0, (rng.uniform(-100, 100), rng.uniform(-100, 100), rng.uniform(-100, 100)), rng.uniform(0.0, 1e4))
    return tree, tracks


def test_properties_on_two_hundred_random_trees():
    rng = random.Random(20261021)
    sliced = refused = 0
    for _ in range(200):
        tree, tracks = random_tree(rng)
        first = 1 + max(n["identifier"] for n in tree)
        try:
            out, relabel, _ = check(tree, tracks, first)
        except R.Refused:                                               # (descending daughters from the 1 ns offsets, for instance: both must refuse)
            refused += 1
            with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception):
                CV.slice_muons(*to_arrays(tree, tracks), first)
            continue
        inputs = {n["identifier"] for n in tree}
        froms = [a for a, _ in relabel]
        assert froms == sorted(set(froms)) and all(b in inputs for _, b in relabel) and not inputs & set(froms)
        pieces = slices_of(out, relabel)
        assert len(pieces) == len(relabel) and sorted(p["identifier"] for p in pieces) == froms        # every slice exactly one entry
        assert all(p["length"] >= 0.1e-3 for p in pieces)
        to = dict(relabel)
        for m in set(to.values()):
            starts = [p["time"] for p in pieces if to[p["identifier"]] == m]
            assert starts == sorted(starts)
        sliced += bool(relabel)
    assert sliced >= 100 and refused < 50
