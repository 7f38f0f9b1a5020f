"""An independent float64 statement of the muon slicer (include/clsimhip.h: "Muon slicer"), written from the text of the reference's
I3MuonSlicer (private/clsim/util/I3MuonSlicer.cxx:95-493, 531-555): plain Python floats, math.log, the reference's operation order, and
the reference's own shape -- a recursive function over child lists.  The library runs on the same machine and must agree bit for bit.

A node is a dict with the fields of clsimhip_tree_particle: type, shape, x, y, z, time, dx, dy, dz, energy, length, identifier, speed,
parent, flags.  A track is a dict identifier, Ei, Ef, ti, tf."""
import math

C = 0.299792458          # I3Constants::c [m/ns]
MM, KM = 1e-3, 1e3
LOG10 = 2.302585092994046
DARK = 1
MUONS = (13, -13)
COUNTERS = ("off_track", "energy_reset", "stops_before_start", "zero_duration", "long_slice")


class Refused(Exception):
    pass


def hypot3(x, y, z):
    xa, ya, za = abs(x), abs(y), abs(z)
    yz = ya if ya > za else za
    w = xa if xa > yz else yz
    if w == 0.0:
        return 0.0
    return w * math.sqrt((xa / w) * (xa / w) + (ya / w) * (ya / w) + (za / w) * (za / w))


def distance_from_track(p, muon):
    hx, hy, hz = p["x"] - muon["x"], p["y"] - muon["y"], p["z"] - muon["z"]
    s = muon["dx"] * hx + muon["dy"] * hy + muon["dz"] * hz
    x2, y2, z2 = muon["x"] + s * muon["dx"], muon["y"] + s * muon["dy"], muon["z"] + s * muon["dz"]
    return hypot3(x2 - p["x"], y2 - p["y"], z2 - p["z"]), s


def slice_muons(tree, tracks, first_slice_identifier):
    """(out, relabel, counters); raises Refused where the library returns CLSIMHIP_ERR_ARGUMENT"""
    index = {}
    for t in tracks:
        if t["identifier"] in index:
            raise Refused("track twice")
        index[t["identifier"]] = t
    children = [[] for _ in tree]
    for i, node in enumerate(tree):
        if node["parent"] < -1 or node["parent"] >= i:
            raise Refused("parent")
        if node["parent"] >= 0:
            children[node["parent"]].append(i)
    out, relabel, counters = [], [], dict.fromkeys(COUNTERS, 0)

    def append(node, parent):
        out.append(dict(node, parent=parent))
        return len(out) - 1

    def append_slice(muon, at, current_time, current_energy, length):
        from_vertex = (current_time - muon["time"]) * C
        identifier = first_slice_identifier + len(relabel)
        if identifier > 0xFFFFFFFF:
            raise Refused("wrap")
        if length > 1.0 * KM:
            counters["long_slice"] += 1
        append(dict(muon, x=muon["x"] + muon["dx"] * from_vertex, y=muon["y"] + muon["dy"] * from_vertex, z=muon["z"] + muon["dz"] * from_vertex,
                    time=current_time, length=length, energy=current_energy, identifier=identifier), at)
        relabel.append((identifier, muon["identifier"]))

    def walk(i, at):
        p, kids = tree[i], children[i]
        if (not math.isnan(p["length"])) and p["length"] > 0.0 and p["type"] in MUONS:
            if any(tree[k]["type"] in MUONS or tree[k]["type"] == 0 for k in kids):
                raise Refused("muon below muon")
            if math.isnan(p["speed"]) or math.isnan(p["energy"]) or math.isnan(p["time"]):
                raise Refused("nan")
            ti = Ei = tf = Ef = math.nan
            if p["identifier"] in index:
                t = index[p["identifier"]]
                ti, Ei, tf, Ef = t["ti"], t["Ei"], t["tf"], t["Ef"]
            # sorted in time, as the reference's helper is meant: the first is no NaN, none is below its predecessor
            for n, k in enumerate(kids):
                if (n == 0 and math.isnan(tree[k]["time"])) or (n > 0 and tree[k]["time"] < tree[kids[n - 1]]["time"]):
                    raise Refused("not sorted")
            bad_ei = bad_ef = False
            if Ei <= 0.0 or math.isnan(Ei):
                Ei, ti, bad_ei = p["energy"], p["time"], True
            if Ef < 0.0 or math.isnan(Ef):
                Ef, tf, bad_ef = 0.0, p["time"] + p["length"] / p["speed"], True
            if math.isnan(ti) or math.isnan(tf):
                raise Refused("t is NaN")
            if Ei <= 0:
                if kids:
                    raise Refused("no energy but children")
            elif tf < ti:
                counters["stops_before_start"] += 1
                out[at]["flags"] |= DARK
            elif tf == ti:
                counters["zero_duration"] += 1
                out[at]["flags"] |= DARK
            else:
                out[at]["flags"] |= DARK
                total = 0.0
                for k in kids:
                    if tree[k]["time"] < ti or tree[k]["time"] > tf:
                        continue
                    total += tree[k]["energy"]
                dEdt_calc = (Ef - Ei + total) / (ti - tf)
                dEdt_max = (0.21 + 8.8e-3 * math.log(Ei / 1.0) / LOG10) * (1.0 / 1.0) * C
                dEdt = min(dEdt_calc, dEdt_max)
                energy, time, iteration = Ei, ti, 0
                for k in kids:
                    d = tree[k]
                    if energy < 0.0:
                        counters["energy_reset"] += 1
                        energy = 0.0
                    off, on = distance_from_track(d, p)
                    if off > 1.0 * MM:
                        counters["off_track"] += 1
                        append(d, at)
                        continue
                    if math.isnan(d["time"]):
                        continue
                    expected = p["time"] + on / p["speed"]
                    duration = expected - time
                    if duration < 0.0:
                        duration = 0.0
                    length = duration * C
                    if length >= 0.1 * MM:
                        append_slice(p, at, time, energy, length)
                    walk(k, append(d, at))
                    time += duration
                    energy -= d["energy"] + dEdt * duration
                    iteration += 1
                if iteration == 0 and bad_ei and bad_ef:
                    return
                if energy < 0.0:
                    return
                length = (tf - time) * C
                if length <= 0.1 * MM:
                    return
                append_slice(p, at, time, energy, length)
                return
        for k in kids:
            walk(k, append(tree[k], at))

    for i, node in enumerate(tree):
        if node["parent"] < 0:
            walk(i, append(node, -1))
    taken = {identifier for identifier, _ in relabel}
    if any(node["identifier"] in taken for node in tree):
        raise Refused("slice identifier in use")
    return out, relabel, counters
