"""Photon hits on the host: the twin (clsimhip_photon_hits_host) against an independent numpy restatement byte for byte -- records,
series table and the seven counters --, the efficiency rule branch by branch, the nested-hits property of the keyed draw, what the
comparisons need to show anything (stated as assertions), the twin's output through the MCPE merging twin, and the twin as a
stand-alone program under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import frame_photons_common as F
from tests import mcpe_common as M
from tests import mcpe_merge_common as MM
from tests import photon_hits_common as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
INPUTS = M.FIXTURES + ("synthetic",)


def records_of(name):
    """(records, series, DOM strings, DOM OMs)"""
    if name == "synthetic":
        return P.synthetic_records(6000, 3) + (F.DOM_STRINGS, F.DOM_OMS)
    return P.fixture_records(name) + M.all_pairs()


@pytest.mark.parametrize("configuration", P.CONFIGURATIONS)
@pytest.mark.parametrize("name", INPUTS)
def test_twin_equals_numpy(name, configuration):
    records, series, strings, oms = records_of(name)
    s = P.configuration(configuration, strings, oms)
    got = P.maker_of(s).MakeHitsHost(records, series)
    P.same(got, P.numpy_hits(records, series, s))
    # the series partition the records, in input order, and the records carry their entry's IDs
    mcpes, table, counters = got
    assert int(table["count"].sum()) == len(mcpes) and (table["count"] > 0).all()
    owner = np.repeat(np.arange(len(table)), table["count"])
    assert np.array_equal(mcpes["stringID"], table["stringID"][owner]) and np.array_equal(mcpes["omID"], table["omID"][owner])
    key = table["frame"].astype(np.int64) * 2 ** 32 + F.dom_code(table["stringID"], table["omID"])
    assert (np.diff(key) > 0).all()                     # (the inputs' tables ascend in (frame, DOM), and the output keeps their order)
    inner = owner[1:] == owner[:-1]
    t = F.tkey_of(mcpes["time"])
    assert not (inner & (t[1:] < t[:-1])).any() and not (inner & (t[1:] == t[:-1]) & (mcpes["id"][1:] < mcpes["id"][:-1])).any()


def test_the_comparisons_show_something():
    """what the tests above need to be worth anything"""
    # at least 1 000 MCPEs in all over the fixtures, and the check is on (and passes) where the photons were recorded without a pancake
    total = 0
    for name in M.FIXTURES:
        records, series, strings, oms = records_of(name)
        total += len(P.maker_of(P.configuration("check_off", strings, oms)).MakeHitsHost(records, series)[0])
    print("MCPEs over the fixtures: %d" % total)
    assert total >= 1000
    records, series, strings, oms = records_of("lea_no_pancake")
    mcpes, _, counters = P.maker_of(P.configuration("check_on", strings, oms)).MakeHitsHost(records, series)
    assert len(mcpes) > 100 and counters["off_surface"] == 0
    records, series, strings, oms = records_of("lea")
    assert P.maker_of(P.configuration("check_on", strings, oms)).MakeHitsHost(records, series)[2]["off_surface"] == len(records)
    # the correction is live and moves records: under pancake 2 a series comes out in another order than it went in
    records, series, strings, oms = records_of("synthetic")
    s = P.keep_all(strings, oms, pancake=2.0)
    live = records.copy()
    live["weight"] = 1.0
    mcpes, table, counters = P.maker_of(s).MakeHitsHost(live, series)
    assert len(mcpes) == len(live) and np.array_equal(table["count"], series["count"])
    moved = [k for k in range(len(series)) if not np.array_equal(mcpes["id"][table["first"][k]:][:table["count"][k]],
                                                                 live["id"][series["first"][k]:][:series["count"][k]])]
    print("series whose order changes under pancake 2: %d of %d" % (len(moved), len(series)))
    assert len(moved) >= 1
    assert not np.array_equal(mcpes["time"], live["time"])
    # ... and with pancake = oversize it is zero: every time is the record's
    same_times = P.maker_of(P.keep_all(strings, oms)).MakeHitsHost(live, series)[0]
    finite = np.isfinite(live["time"])
    assert np.array_equal(np.sort(same_times["time"][np.isfinite(same_times["time"])]), np.sort(live["time"][finite]))


def crafted():
    """(records, series, spec): synthetic records on the sphere with one of everything"""
    records, series = P.synthetic_records(6000, 3)
    records, series = records.copy(), series.copy()
    strings, oms = F.DOM_STRINGS, F.DOM_OMS
    records["weight"][np.arange(len(records)) % 97 == 5] = -1.0                        # negative weights
    foreign = (strings == series["stringID"][2]) & (oms == series["omID"][2])          # a DOM the maker's table does not have
    series["omID"][5] += 1                                                              # an entry with other IDs than its records
    series = np.delete(series, [0, 9])                                                  # records in front of the table, and a gap in it
    s = P.spec(P.dom_table(strings[~foreign], oms[~foreign], inactive_every=10), tables=[M.acceptance_table(8.0)], pancake=1.0, ignore_inactive=True)
    return records, series, s


def test_every_counter_counts():
    records, series, s = crafted()
    got = P.maker_of(s).MakeHitsHost(records, series)
    print(got[2])
    assert all(got[2][k] > 0 for k in CV.PHOTON_HIT_COUNTERS), got[2]
    assert len(got[0]) > 0
    P.same(got, P.numpy_hits(records, series, s))
    # only_warn: the off-surface records are counted and go on
    warned = P.maker_of(dict(s, only_warn=True)).MakeHitsHost(records, series)
    assert warned[2]["off_surface"] == got[2]["off_surface"] and len(warned[0]) > len(got[0])
    P.same(warned, P.numpy_hits(records, series, dict(s, only_warn=True)))
    # a table that does not ascend is walked by the same bisection in both
    shuffled = series[np.random.default_rng(5).permutation(len(series))]
    got = P.maker_of(s).MakeHitsHost(records, shuffled)
    assert got[2]["uncovered"] > 0
    P.same(got, P.numpy_hits(records, shuffled, s))
    # no records; no series table
    P.same(P.maker_of(s).MakeHitsHost(records[:0], series), P.numpy_hits(records[:0], series, s))
    empty = P.maker_of(s).MakeHitsHost(records, series[:0])
    assert empty[2]["uncovered"] == len(records) and len(empty[0]) == 0
    P.same(empty, P.numpy_hits(records, series[:0], s))


@pytest.mark.parametrize("configuration", ["check_on", "rotated", "warn_on", "efficiencies"])
def test_adversarial_patterns(configuration):
    """NaN, +-inf, denormals and huge angles in every float field, NaN times, zero group velocities"""
    records, series = P.adversarial_records(6000, 4)
    for name in F.FLOATS:
        assert np.isnan(records[name]).sum() >= 10 and np.isinf(records[name]).sum() >= 10
    assert np.isnan(records["time"]).sum() >= 10 and (records["groupVelocity"] == 0).sum() >= 100
    s = P.configuration(configuration, F.DOM_STRINGS, F.DOM_OMS)
    got = P.maker_of(s).MakeHitsHost(records, series)
    P.same(got, P.numpy_hits(records, series, s))
    # every NaN time of the output has the one pattern
    nan = np.isnan(got[0]["time"])
    assert nan.sum() >= 1 and (got[0]["time"].view(np.uint64)[nan] == 0x7ff8000000000000).all()


# ---- the efficiency rule ----
def one_dom(flags=CV.PHOTON_HIT_HAS_STATUS | CV.PHOTON_HIT_IN_CALIBRATION, eff=0.8, spe=1.25):
    d = P.dom_table([12, 12], [7, 8])
    d["flags"][1], d["relativeDOMEff"][1], d["speCompensationFactor"][1] = flags, eff, spe
    return d


RULE = {    # name: (DOM, configuration, the efficiency)
    "replace": (one_dom(), dict(default=0.7, replace=True), 0.7),
    "not_in_calibration": (one_dom(flags=CV.PHOTON_HIT_HAS_STATUS), dict(default=0.6), 0.6),
    "nan_efficiency": (one_dom(eff=P.NAN), dict(default=0.55), 0.55),                  # the default WITHOUT the SPE factor
    "nan_spe_factor": (one_dom(spe=P.NAN), dict(default=0.3), 0.8),
    "product": (one_dom(eff=0.1, spe=3.0), dict(default=0.3), 0.1 * 3.0),
    "product_without_a_default": (one_dom(), dict(), 0.8 * 1.25),
    "default_zero": (one_dom(), dict(default=0.0, replace=True), 0.0),
}


@pytest.mark.parametrize("name", sorted(RULE))
def test_efficiency_rule(name):
    doms, kwargs, want = RULE[name]
    s = P.spec(doms, **kwargs)
    maker = P.maker_of(s)
    assert maker.Efficiency(12, 8) == want == P.resolve_efficiency(s)[1]
    assert maker.Efficiency(12, 7) == (kwargs["default"] if kwargs.get("replace") else 1.0)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=r"OM \(12/9\) is not in the DOM table") as e:
        maker.Efficiency(12, 9)
    assert e.value.code == _lib.ERR_ARGUMENT


REFUSED = {  # name: (DOM, configuration, the text)
    "replace_with_a_nan_default": (one_dom(), dict(replace=True), r"OM \(12/7\): You need to set \"DefaultRelativeDOMEfficiency\" to a value other than NaN"),
    "not_in_calibration": (one_dom(flags=0), dict(), r"OM \(12/8\) not found in the current calibration map! \(Consider setting"),
    "nan_efficiency": (one_dom(eff=P.NAN), dict(), r"OM \(12/8\) found in the current calibration map, but it is NaN!"),
    "negative_default": (one_dom(), dict(default=-0.5), r"The \"DefaultRelativeDOMEfficiency\" parameter must not be < 0!"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_efficiency_rule_refuses_what_the_reference_ends_on(name):
    doms, kwargs, text = REFUSED[name]
    s = P.spec(doms, **kwargs)
    with pytest.raises(ValueError):
        P.resolve_efficiency(s)
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match=text) as e:
        P.maker_of(s)
    assert e.value.code == _lib.ERR_CONFIG


def test_creation_refuses_bad_tables():
    good = P.dom_table([1, 1], [1, 2])
    for change, code in ((dict(stringID=40000), _lib.ERR_ARGUMENT), (dict(stringID=-40000), _lib.ERR_ARGUMENT), (dict(omID=70000), _lib.ERR_ARGUMENT),
                         (dict(omID=1), _lib.ERR_ARGUMENT),            # a pair named twice
                         (dict(classIndex=1), _lib.ERR_ARGUMENT), (dict(flags=4), _lib.ERR_ARGUMENT)):
        d = good.copy()
        for k, v in change.items():
            d[k][1] = v
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            P.maker_of(P.spec(d))
        assert e.value.code == code, change
    for kwargs in (dict(pancake=0.0), dict(oversize=float("inf")), dict(dom_radius=-1.0), dict(coefficients=np.ones(33)),
                   dict(tables=[M.acceptance_table()] * 9)):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            P.maker_of(P.spec(good, **kwargs))
        assert e.value.code == _lib.ERR_ARGUMENT, kwargs
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="more than 4096 values") as e:
        P.maker_of(P.spec(good, tables=[(3e-7, 1e-9, np.ones(4097))]))
    assert e.value.code == _lib.ERR_CONFIG
    # the limits themselves are fine: 8 classes, 4 096 values, 32 coefficients
    P.maker_of(P.spec(good, tables=[(3e-7, 1e-9, np.ones(512))] * 8, coefficients=np.ones(32)))


# ---- common random numbers ----
def as_multiset(mcpes):
    return sorted(m.tobytes() for m in mcpes)


def test_hits_at_a_lower_efficiency_are_a_subset_with_the_same_seed():
    """pancake = oversize: the records at efficiency 0.5 are a sub-multiset of those at 1.0; another seed gives another set"""
    records, series, strings, oms = records_of("flasher_led405")
    half = P.maker_of(P.spec(P.dom_table(strings, oms, efficiencies=(0.5,)))).MakeHitsHost(records, series)[0]
    full = P.maker_of(P.spec(P.dom_table(strings, oms, efficiencies=(1.0,)))).MakeHitsHost(records, series)[0]
    other = P.maker_of(P.spec(P.dom_table(strings, oms, efficiencies=(0.5,)), seed=P.SEED + 1)).MakeHitsHost(records, series)[0]
    assert 100 < len(half) < len(full)
    remaining = as_multiset(full)
    from collections import Counter
    assert not Counter(as_multiset(half)) - Counter(remaining)
    assert Counter(as_multiset(other)) - Counter(remaining)            # the other seed's hits are not a subset
    assert as_multiset(other) != as_multiset(half) and abs(len(other) - len(half)) < 0.2 * len(half)


# ---- chaining ----
@pytest.mark.parametrize("name", ["flasher_led405", "synthetic"])
def test_the_output_goes_into_the_merging_twin(name):
    records, series, strings, oms = records_of(name)
    s = P.configuration("correction_live", strings, oms) if name != "synthetic" else P.keep_all(strings, oms, pancake=2.0)
    if name == "synthetic":
        records = records.copy()
        records["weight"] = 1.0
    mcpes, table, _ = P.maker_of(s).MakeHitsHost(records, series)
    assert len(mcpes) > 1000
    for window in (0.0, 5.0, 200.0):
        got = CV.MCPEGenerator.MergeHost(mcpes, table, window)
        MM.same(got, MM.numpy_merge(mcpes, table, window))
        MM.check_properties(mcpes, table, window, got)
    assert len(CV.MCPEGenerator.MergeHost(mcpes, table, 200.0)[0]) < len(mcpes)


# ---- the C structs ----
def test_struct_layouts_match_the_header(tmp_path):
    dom = ["string_id", "om_id", "class_index", "flags", "relative_dom_eff", "spe_compensation_factor", "dir_x"]
    config = ["dom_radius", "oversize", "pancake", "default_relative_efficiency", "replace_efficiency_with_default", "ignore_inactive",
              "only_warn_off_surface", "reserved", "seed"]
    counters = ["UNCOVERED", "SERIES_MISMATCH", "UNKNOWN_DOM", "INACTIVE", "NEGATIVE_WEIGHT", "OFF_SURFACE", "PROBABILITY_ABOVE_ONE"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "clsimhip.h"', "int main(void) {",
             'printf("%zu %zu\\n", sizeof(clsimhip_photon_hit_dom), sizeof(clsimhip_photon_hit_config));']
    lines += ['printf("%%zu\\n", offsetof(clsimhip_photon_hit_dom, %s));' % k for k in dom]
    lines += ['printf("%%zu\\n", offsetof(clsimhip_photon_hit_config, %s));' % k for k in config]
    lines += ['printf("%%d\\n", CLSIMHIP_PHOTON_HITS_%s);' % k for k in counters]
    lines += ['printf("%u %u\\n", CLSIMHIP_PHOTON_HITS_FLAG_HAS_STATUS, CLSIMHIP_PHOTON_HITS_FLAG_IN_CALIBRATION);', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    words = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    d, c = CV.PHOTON_HIT_DOM_DTYPE, _lib.PhotonHitConfig
    assert words == ([d.itemsize, _lib.C.sizeof(c)] + [d.fields[k][1] for k in d.names] + [getattr(c, k).offset for k, _ in c._fields_] +
                     [CV.PHOTON_HIT_COUNTERS.index(k.lower()) for k in counters] + [CV.PHOTON_HIT_HAS_STATUS, CV.PHOTON_HIT_IN_CALIBRATION])


# ---- the twin as a program of its own, under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/photon_hits_host_main.cpp with clsim_amd/csrc/photon_hits.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("photon_hits_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    sources = [os.path.join(ROOT, "clsim_amd", "csrc", "photon_hits.cpp"), os.path.join(ROOT, "tests", "photon_hits_host_main.cpp")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c"] + sources, cwd=str(d))
    exe = str(d / "photon_hits_host_main")
    # (linked without the HIP runtime: the program defines the entry points the file names)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "photon_hits.o",
                           "photon_hits_host_main.o", "-o", exe], cwd=str(d))
    return exe


def run_host_program(exe, tmp_path, records, series, s):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    P.write_input(src, records, series, s)
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    return run, (np.fromfile(dst, dtype=np.uint8) if run.returncode == 0 else None)


def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path):
    crafted_records, crafted_series, crafted_spec = crafted()
    adversarial = P.adversarial_records(6000, 4)
    live = P.synthetic_records(6000, 3)[0].copy()
    live["weight"] = 1.0
    cases = [(crafted_records, crafted_series, crafted_spec), (crafted_records, crafted_series[::-1].copy(), crafted_spec),
             adversarial + (P.configuration("rotated", F.DOM_STRINGS, F.DOM_OMS),), adversarial + (P.configuration("warn_on", F.DOM_STRINGS, F.DOM_OMS),),
             (live, P.synthetic_records(6000, 3)[1], P.keep_all(F.DOM_STRINGS, F.DOM_OMS, pancake=2.0)),
             (crafted_records[:0], crafted_series, crafted_spec), (crafted_records, crafted_series[:0], crafted_spec)]
    for records, series, s in cases:
        want = P.maker_of(s).MakeHitsHost(records, series)
        run, out = run_host_program(host_program, tmp_path, records, series, s)
        assert run.returncode == 0 and not run.stderr, run.stderr
        assert run.stdout.split() == ["kept", str(len(want[0])), "series", str(len(want[1])), "counters"] + [str(want[2][k]) for k in CV.PHOTON_HIT_COUNTERS]
        assert out.tobytes() == want[0].tobytes() + want[1].tobytes()
    # a configuration the reference ends on: an error message and exit code 1, not a crash
    run, _ = run_host_program(host_program, tmp_path, crafted_records, crafted_series, dict(crafted_spec, default=-1.0))
    assert run.returncode == 1 and "must not be < 0" in run.stderr
