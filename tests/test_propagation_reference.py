"""The ORACLE against the float64 statements of tests/propagation_reference.py (CPU only): how the full detector's DOM search and the
layer walk assemble their pieces.  Every other propagation test compares product and oracle bit for bit, and the oracle restates the
reference's kernel and geometry builder line by line -- a mistake shared by both restatements shows only against a statement that
shares nothing with them.  tests/test_propagation_reference_gpu.py runs the same inputs and assertions on the kernels.

Clear-ice rays: flasher steps of one photon in ice with absorption and scattering lengths of 1e7 m; the photon is the ray (step
position, step direction), and the first DOM on it, by brute force over every DOM, is the record.  Layer walk: cascade bunches with
photon histories; between two recorded points the history's fourth component grows by the statement's path integral.

The bounds are derived in tests/propagation_reference.py, none is fitted; what is asserted is four times the first order bound, and
HEADROOM holds the oracle to the first order bound itself.  Measured on the oracle, worst error / ASSERTED bound over all cases (each
test prints its own, with the shares of fragile rays, rays left out by draws and flat segments):
    rays: cherenkovDist 0.169, time 0.168, position 0.140, radius 0.128, groupVelocity 0.116, weight 0.079, theta 0.059, phi 0.083;
          fragile 0.75 ... 0.93 % of a bunch, left out by draws 0.024 ... 0.055 %, at least 245 decided rays in every class;
    walk: segment 0.164 (SPICE-Lea, 2.2e-5 absorption lengths; Mie 1.2e-6, photonics 1.0e-6, constants 4.1e-6), path length 0.013,
          time of flight 0.069, groupVelocity 0.142, weight 0.112, position 0.009; no flat segment; 85 ... 89 % complete paths.
LABBOOK.md, "Propagation against float64 statements", has the error against distance of the search."""
import numpy as np
import pytest

from tests import propagation_common as PC
from tests import propagation_reference as PR

HEADROOM = 0.25          # the oracle's worst error stays under a quarter of every derived bound


def report(what, worst):
    print("%s: worst error / bound: %s" % (what, ", ".join("%s %.3g" % (k, v) for k, v in worst.items())))


@pytest.mark.parametrize("pancake", [1.0, 5.0])
@pytest.mark.parametrize("geom", ["ic86", "regular", "60", "large"])
def test_clear_ice_rays_hit_the_first_dom_of_the_brute_force_search(oracle_lib, geom, pancake):
    """every decided ray is detected exactly when the statement says so, on that DOM, with that record.  The far class (300 ... 1500 m)
    holds the error to E(s): at 750 m the reference's search decides impact parameters to about +-0.2 m only."""
    case = PC.ray_case(geom, pancake)
    what = "%s, pancake %g" % (geom, pancake)
    worst = PC.check_rays(case, PC.oracle_rays(case), what)
    print(what + ": " + PC.caps_message(case))
    report(what, worst)
    assert all(v <= HEADROOM for v in worst.values()), worst
    st = case["st"]
    far = case["decided"] & st["hit"] & (case["cls"] == PC.CLASSES.index("far"))
    assert far.sum() >= 100 and np.sqrt(st["r2"][far]).max() > 400.0
    inside = st["inside"] & (case["cls"] == PC.CLASSES.index("inside"))
    # the class of its own: not detected on the DOM they start in (the ellipsoid flattened along the ray holds 1 / pancake of the sphere)
    assert inside.sum() >= (1000 if pancake == 1.0 else 100)


def test_clear_ice_rays_without_stopping_give_every_single_dom_its_record(oracle_lib):
    case = PC.ray_case("60", 5.0)
    T = PC.oracle_tables_for(case["geom"], PC.clear_medium_o(), True, 5.0, stop_detected=False)
    from oracle import capi
    x, a = case["streams"]
    ph, cnt, _, _ = capi.propagate(T, case["steps"], x, a, threads=1, max_hits=8 * PC.N_RAYS)
    assert cnt == len(ph)
    worst = PC.check_rays_kept(case, capi.replace_indices_with_ids(ph, T.geo), "60, kept")
    report("60, kept", worst)


@pytest.mark.parametrize("name", PC.WALK_MEDIA)
def test_layer_walk_uses_up_the_path_integral_of_the_statement(oracle_lib, name):
    """between two recorded scatter points the history's fourth component grows by sum (path in layer) / absLen / anisotropy factor
    with the tilt taken at the segment's start; the last stretch to the DOM uses up at least the integral up to the hit"""
    ph, hist = PC.oracle_walk(name)
    worst = PC.check_walk(name, ph, hist, name)
    report(name, worst)
    for k in ("segment", "last stretch", "path length", "position", "radius", "weight", "groupVelocity", "time of flight"):
        assert worst[k] <= HEADROOM, (k, worst)


def test_statement_of_the_walk_on_hand_made_segments():
    """the statement itself on segments whose integral can be written down: one layer, two layers, below the lowest layer"""
    med = dict(num_layers=3, layers_z_start=-10.0, layers_height=10.0, len_mode="constant", abs_const=np.array([10.0, 20.0, 40.0]))
    used, bound, flat, crossings = PR.absorption_lengths_used(med, [0.0, 0.0, -5.0], [3.0, 4.0, -5.0 + 1e-9], 4e-7)
    assert flat and used == pytest.approx(5.0 / 10.0)
    used, bound, flat, crossings = PR.absorption_lengths_used(med, [0.0, 0.0, -5.0], [0.0, 0.0, 15.0], 4e-7)
    assert not flat and crossings == 2 and used == pytest.approx(5.0 / 10.0 + 10.0 / 20.0 + 5.0 / 40.0) and bound < 1e-4
    used, _, _, crossings = PR.absorption_lengths_used(med, [0.0, 0.0, 25.0], [30.0, 0.0, -15.0], 4e-7)        # 50 m long, 40 m down
    assert crossings == 2 and used == pytest.approx((50.0 / 40.0) * (15.0 / 40.0 + 10.0 / 20.0 + 15.0 / 10.0))
    used, _, _, crossings = PR.absorption_lengths_used(med, [0.0, 0.0, -30.0], [0.0, 0.0, -20.0], 4e-7)        # the outermost layers go on
    assert crossings == 0 and used == pytest.approx(1.0)
