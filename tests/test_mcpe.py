"""MCPE generator, host side: the host twin of the hit maker (clsimhip_mcpe_convert_host) against an independent numpy
restatement of the definition in include/clsimhip.h, on the committed photon records of six configurations; the four
conditions the reference ends the run on; the configuration errors.  No GPU here (tests/test_mcpe_gpu.py has the kernel)."""
import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import common
from tests import mcpe_common as M


def one_class(strings, doms):
    return np.zeros(len(strings), dtype=np.int64)


def counters_of(**kw):
    return dict(dict.fromkeys(CV.MCPE_CONDITIONS, 0), **kw)


@pytest.mark.parametrize("name", M.FIXTURES)
def test_host_twin_equals_numpy_restatement(name):
    ph = M.fixture_photons(name)
    pancake = M.pancake_of(name)
    got, counters = M.standard_generator(pancake).ConvertHost(ph)
    want, want_counters, P, accepted = M.numpy_mcpes(ph, [M.acceptance_table()], one_class, M.angular_coefficients(), pancake)
    assert counters == want_counters == counters_of()
    assert len(got) == len(want) > 0
    assert got.tobytes() == want.tobytes()              # same records, same order, same bits
    if name == "lea_no_pancake":
        # pancake 1 with oversize 5: records sit at r = 0.8255 m and the arrival time correction is not zero
        assert np.any(got["time"] != ph["t"][accepted].astype(np.float64))
        r = np.sqrt(sum(ph[k].astype(np.float64) ** 2 for k in "xyz"))
        assert np.abs(r - 0.8255).max() < 0.03
    else:
        assert np.array_equal(got["time"], ph["t"][accepted].astype(np.float64))


@pytest.mark.parametrize("name", M.FIXTURES)
def test_accepted_count_follows_the_probabilities(name):
    """accepted count within 4 binomial sigma of the sum of P; P stays inside (0, 1); no fixture holds a record twice (two equal
    records would share their draw)"""
    ph = M.fixture_photons(name)
    got, _ = M.standard_generator(M.pancake_of(name)).ConvertHost(ph)
    _, _, P, _ = M.numpy_mcpes(ph, [M.acceptance_table()], one_class, M.angular_coefficients(), M.pancake_of(name))
    assert len(P) == len(ph) and 0.004 < P.min() and P.max() < 0.75
    sigma = np.sqrt(np.sum(P * (1.0 - P)))
    print("%s: %d records, accepted %d, sum P %.1f, sigma %.2f, P in [%.4f, %.3f]" % (name, len(ph), len(got), P.sum(), sigma, P.min(), P.max()))
    assert abs(len(got) - P.sum()) < 4.0 * sigma
    assert len(np.unique(ph.view(np.uint8).reshape(len(ph), 80), axis=0)) == len(ph)


def test_draw_depends_on_the_seed_and_on_nothing_else():
    ph = M.fixture_photons("mie")
    a, _ = M.standard_generator(seed=1).ConvertHost(ph)
    b, _ = M.standard_generator(seed=2).ConvertHost(ph)
    assert a.tobytes() != b.tobytes()
    # a permuted input gives the permuted output: the draw is keyed on the record, not on its place
    order = np.random.default_rng(5).permutation(len(ph))
    c, _ = M.standard_generator(seed=1).ConvertHost(ph[order])
    assert M.sort_mcpes(c).tobytes() == M.sort_mcpes(a).tobytes()


@pytest.mark.parametrize("name,on_dense", [("mie", 106), ("lea", 111), ("lea_no_pancake", 118)])
def test_two_classes(name, on_dense):
    """IceCube / DeepCore in the reference's I3CLSimFunctionMap: the second class is half the table, on strings >= 79"""
    ph = M.fixture_photons(name)
    pancake = M.pancake_of(name)
    assert int((ph["stringID"] >= 79).sum()) == on_dense
    tables = [M.acceptance_table(), M.acceptance_table(0.5)]
    s, d = M.all_pairs()
    gen = M.make_generator(tables, s, d, (s >= 79).astype(np.int32), pancake=pancake)
    got, counters = gen.ConvertHost(ph)
    want, want_counters, _, _ = M.numpy_mcpes(ph, tables, lambda strings, doms: (strings >= 79).astype(np.int64), M.angular_coefficients(), pancake)
    assert counters == want_counters == counters_of()
    assert got.tobytes() == want.tobytes()
    assert (got["stringID"] >= 79).any() and (got["stringID"] < 79).any()
    one, _ = M.standard_generator(pancake).ConvertHost(ph)
    assert len(one) != len(got) or one.tobytes() != got.tobytes()       # the second class is not the first


def test_negative_weight_is_counted_and_zero_weight_is_dropped():
    ph = M.fixture_photons("mie")
    ph["weight"][::7] *= -1.0
    ph["weight"][3::7] = 0.0
    got, counters = M.standard_generator().ConvertHost(ph)
    want, want_counters, P, _ = M.numpy_mcpes(ph, [M.acceptance_table()], one_class, M.angular_coefficients(), 5.0)
    assert counters == want_counters == counters_of(negative_weight=len(ph[::7]))
    assert len(P) == len(ph) - len(ph[::7]) - len(ph[3::7])
    assert got.tobytes() == want.tobytes() and len(got) > 0


def test_probability_above_one_is_counted():
    ph = M.fixture_photons("mie")
    table = M.acceptance_table(2.0)
    s, d = M.all_pairs()
    got, counters = M.make_generator([table], s, d, np.zeros(len(s), dtype=np.int32)).ConvertHost(ph)
    want, want_counters, _, _ = M.numpy_mcpes(ph, [table], one_class, M.angular_coefficients(), 5.0)
    assert counters == want_counters and counters["probability_above_one"] > 0
    assert counters == counters_of(probability_above_one=counters["probability_above_one"])
    assert got.tobytes() == want.tobytes()


def test_records_off_the_surface_are_counted():
    ph = M.fixture_photons("lea_no_pancake")            # recorded at r = 5 x 0.1651 m; the generator expects 0.1651 m
    got, counters = M.standard_generator(pancake=5.0).ConvertHost(ph)
    want, want_counters, _, _ = M.numpy_mcpes(ph, [M.acceptance_table()], one_class, M.angular_coefficients(), 5.0)
    assert len(got) == len(want) == 0
    assert counters == want_counters == counters_of(off_surface=len(ph))


def test_dom_without_class_is_counted():
    ph = M.fixture_photons("mie")
    s, d = M.all_pairs()
    known = s != ph["stringID"][0]
    gen = M.make_generator([M.acceptance_table()], s[known], d[known], np.zeros(int(known.sum()), dtype=np.int32))
    got, counters = gen.ConvertHost(ph)
    want, want_counters, _, _ = M.numpy_mcpes(ph, [M.acceptance_table()], lambda strings, doms: np.where(strings == ph["stringID"][0], -1, 0),
                                              M.angular_coefficients(), 5.0)
    assert counters == want_counters == counters_of(unknown_dom=int((ph["stringID"] == ph["stringID"][0]).sum()))
    assert got.tobytes() == want.tobytes()


def test_ids_of_any_sign_and_size_find_their_class():
    """the class table takes any int16 / uint16 pair"""
    ph = M.fixture_photons("mie")
    ph["stringID"] = np.where(ph["stringID"] % 2 == 0, -ph["stringID"] - 1, ph["stringID"] + 30000)
    ph["omID"] = ph["omID"] + 65000
    s, d = M.all_pairs()
    s2 = np.where(s % 2 == 0, -s - 1, s + 30000).astype(np.int32)
    gen = M.make_generator([M.acceptance_table()], s2, d + 65000, np.zeros(len(s), dtype=np.int32))
    got, counters = gen.ConvertHost(ph)
    want, _, _, _ = M.numpy_mcpes(ph, [M.acceptance_table()], one_class, M.angular_coefficients(), 5.0)
    assert counters == counters_of() and got.tobytes() == want.tobytes() and (got["stringID"] < 0).any()


def test_angles_outside_zero_to_two_pi():
    """records from elsewhere may carry any angle: outside [0, 2 pi] the device math library takes its Cephes form, which no
    propagated record reaches (theta in [0, pi], phi in [0, 2 pi])"""
    ph = np.concatenate([M.fixture_photons("mie"), M.fixture_photons("lea")])
    two_pi = np.float32(2.0 * np.pi)
    k = np.arange(len(ph))
    # the same directions under other names: phi - 2 pi, phi + 2 pi k, and (-theta, phi + pi)
    ph["phi"] = np.where(k % 3 == 0, ph["phi"] - two_pi, np.where(k % 3 == 1, ph["phi"] + two_pi * (1 + k % 5), ph["phi"])).astype(np.float32)
    flip = k % 4 == 0
    ph["theta"] = np.where(flip, -ph["theta"], ph["theta"])
    ph["phi"] = np.where(flip, ph["phi"] + np.float32(np.pi), ph["phi"]).astype(np.float32)
    outside = (ph["phi"] < 0) | (ph["phi"] > two_pi) | (ph["theta"] < 0)
    assert outside.sum() > len(ph) // 2 and (ph["phi"] < 0).any() and (ph["phi"] > 7).any() and (ph["theta"] < 0).any()
    got, counters = M.standard_generator().ConvertHost(ph)
    want, want_counters, _, _ = M.numpy_mcpes(ph, [M.acceptance_table()], one_class, M.angular_coefficients(), 5.0)
    assert counters == want_counters == counters_of()
    assert got.tobytes() == want.tobytes() and len(got) > 300


def test_capacity_smaller_than_the_result_counts_on():
    import ctypes as C
    ph = M.fixture_photons("mie")
    gen = M.standard_generator()
    full, _ = gen.ConvertHost(ph)
    out = np.zeros(10, dtype=CV.MCPE_DTYPE)
    n = C.c_size_t()
    rc = _lib.load().clsimhip_mcpe_convert_host(gen._h, ph.ctypes.data_as(C.c_void_p), len(ph), out.ctypes.data_as(C.c_void_p), 10, C.byref(n), None)
    assert rc == 0 and n.value == len(full) > 10 and out.tobytes() == full[:10].tobytes()


def test_only_tables_with_equal_spacing_and_constants_are_classes():
    s, d = M.all_pairs()
    start, step, values = M.acceptance_table()
    poly = M.I3CLSimFunctionPolynomial(M.angular_coefficients())
    for bad in (CV.I3CLSimFunctionFromTable(start + step * np.arange(len(values)), values), CV.I3CLSimFunctionDeltaPeak(4e-7)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            CV.MCPEGenerator([bad], s, d, np.zeros(len(s), dtype=np.int32), poly)
        assert e.value.code == _lib.ERR_CONFIG
    # a constant is one
    gen = CV.MCPEGenerator([CV.I3CLSimFunctionConstant(2e-3)], s, d, np.zeros(len(s), dtype=np.int32), poly, domRadius=M.DOM_RADIUS,
                           oversizeFactor=5.0, pancakeFactor=5.0, seed=M.SEED)
    ph = M.fixture_photons("mie")
    got, counters = gen.ConvertHost(ph)
    # (for the restatement a constant is a table of two equal values)
    want, want_counters, _, _ = M.numpy_mcpes(ph, [(start, step, np.array([2e-3, 2e-3]))], one_class, M.angular_coefficients(), 5.0)
    assert counters == want_counters and got.tobytes() == want.tobytes() and 0 < len(got) < len(ph)


def test_compile_refuses_a_dom_without_class():
    cfg = common.config("c1")
    g = cfg["geom"]
    ids_s, ids_d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    conv = common.product_converter(cfg, 512, initialize=False)
    gen = M.make_generator([M.acceptance_table()], ids_s[1:], ids_d[1:], np.zeros(len(ids_s) - 1, dtype=np.int32))
    conv.SetMCPEGenerator(gen, True)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="No wavelength acceptance") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
    # with every DOM named, and with the generator taken off again, it compiles
    conv.SetMCPEGenerator(M.make_generator([M.acceptance_table()], ids_s, ids_d, np.zeros(len(ids_s), dtype=np.int32)), False)
    conv.Compile()
    conv.SetMCPEGenerator(None)
    conv.Compile()


def test_compile_refuses_another_pancake_factor_and_histories_without_photons():
    cfg = common.config("c1")
    g = cfg["geom"]
    ids_s, ids_d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    zero = np.zeros(len(ids_s), dtype=np.int32)
    conv = common.product_converter(cfg, 512, initialize=False)            # pancake factor 5
    conv.SetMCPEGenerator(M.make_generator([M.acceptance_table()], ids_s, ids_d, zero, pancake=1.0), True)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="pancake factor") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
    gen = M.make_generator([M.acceptance_table()], ids_s, ids_d, zero, pancake=5.0)
    conv.SetMCPEGenerator(gen, False)
    conv.SetPhotonHistoryEntries(4)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="photon histories need keep_photons") as e:
        conv.Compile()
    assert e.value.code == _lib.ERR_CONFIG
    conv.SetMCPEGenerator(gen, True)
    conv.Compile()


def test_design_quotes_the_record_sizes():
    """DESIGN.md section 8 quotes the traffic of the MCPE kernel from the record sizes"""
    assert CV.MCPE_DTYPE.itemsize == 16 and M.PHOTON_DTYPE.itemsize == 80
    assert abs(184363 * (80 + 16) / 1e6 - 17.7) < 0.05


def test_design_quotes_the_host_twin_rate():
    """the host twin makes 1.0 ... 1.3e7 records per second on one thread (tools/mcpe_host_rate.py), more than
    the 3.7e6 per second one GPU delivers.  Timing on a shared machine: only the order of magnitude is asserted (a twentieth)."""
    import time
    ph = np.tile(np.concatenate([M.fixture_photons(n) for n in ("mie", "lea", "flasher_led405")]), 30)
    gen = M.standard_generator()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        got, counters = gen.ConvertHost(ph)
        best = min(best, time.perf_counter() - t0)
    print("host twin: %.3g records per second" % (len(ph) / best))
    assert counters == counters_of() and len(ph) / best > 5e5
