"""Series relabel on the host: the twins (clsimhip_mcpe_series_relabel_host / clsimhip_frame_photons_relabel_host) against the numpy
statement of RELABEL in tests/series_relabel_common.py, byte for byte and for both record types; the bridges to the series stage, the
merging stage and the union (P1 ... P4) on inputs asserted to hold a disturbed run; the parent table; every refusal; and the host
code of the slicer and of this stage as a stand-alone program under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import series_relabel_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def check(kind, records, series, m):
    want = R.numpy_relabel(kind, records, series, m)
    got = R.host(kind, records, series, m)
    R.same(got, want)
    return got


@pytest.mark.parametrize("kind", R.KINDS)
def test_small_inputs_and_maps(kind):
    empty = np.zeros(0, dtype=R.DTYPE[kind]), np.zeros(0, dtype=CV.MCPE_SERIES_DTYPE)
    assert check(kind, *empty, R.relabel_map([(5, 1)]))[2] == (0, 0, 0, 0, 0)
    one = R.form_of(kind, R.blank(kind, 1), np.zeros(1, dtype=np.uint32))
    one[0]["id"] = 5
    assert check(kind, *one, R.relabel_map([(5, 1)]))[0]["id"][0] == 1
    records, series, m = R.run_case(kind, 64, True)
    got = check(kind, records, series, m[:0])                           # an empty map: a copy
    assert got[0].tobytes() == records.tobytes() and got[2][2] == 0
    got = check(kind, records, series, R.relabel_map([(7, 1), (2000, 2)]))          # a map that names no record
    assert got[0].tobytes() == records.tobytes() and got[2][2] == 0
    got = check(kind, *R.extreme_identifiers_case(kind))
    assert got[2][2] == 4 and list(got[0]["id"]) == [1, 5, 0xFFFFFFFE] * 2


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("length", R.RUNS)
@pytest.mark.parametrize("disturbed", (False, True))
def test_runs_of_equal_times(kind, length, disturbed):
    records, series, m = R.run_case(kind, length, disturbed)
    r = records.copy()
    r["id"], _ = R.new_ids(r["id"], m)
    assert (len(R.disturbed_runs(kind, r, series)[0]) == 1) == (disturbed and length >= 2)
    got = check(kind, records, series, m)
    overflows = disturbed and length > R.BOUND
    assert (got[2][4] == length) if overflows else (got[2][4] == 0 and got[2][0] == len(records))
    assert got[2][2] == int((records["id"] == 1005).sum() + (records["id"] == 1009).sum())


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_long_undisturbed_run_is_copied(kind):
    records, series, m = R.run_case(kind, 5000, False)
    got = check(kind, records, series, m)
    assert got[2][0] == 5006 and got[2][4] == 0


@pytest.mark.parametrize("kind", R.KINDS)
def test_boundaries_zeros_nans_and_duplicates(kind):
    got = check(kind, *R.boundary_case(kind))
    assert list(got[0]["id"]) == [1000, 1001, 1000, 1001]               # joined, the runs would give 1000, 1000, 1001, 1001
    got = check(kind, *R.zero_and_nan_case(kind))
    assert list(got[0]["id"]) == [1000, 1000, 1001, 1000, 1002, 1000, 1001, 1000]     # -NaN | -0.0 | +0.0 | NaN | another NaN
    got = check(kind, *R.duplicates_case(kind))
    assert list(got[0]["id"]) == [1001, 1001, 1001, 1001, 1003]
    assert len({got[0][k].tobytes() for k in range(4)}) == 1


@pytest.fixture(scope="module", params=R.KINDS)
def forms(request):
    """per record type: the stage, and three random forms with their raw records"""
    kind = request.param
    stage = R.stage_of(kind)
    return kind, stage, [R.random_form(kind, stage, n, seed) for n, seed in ((6000, 3), (9000, 4), (2500, 5))]


def test_p1_relabel_of_the_series_is_the_series_of_the_relabelled(forms):
    kind, stage, made = forms
    for raw, records, series in made:
        assert R.has_a_disturbed_run(kind, records, series, R.SLICE_MAP)
        got = check(kind, records, series, R.SLICE_MAP)
        at_source = raw.copy()
        at_source["id"], _ = R.new_ids(at_source["id"], R.SLICE_MAP)
        want = R.series_of(kind, stage, at_source)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_p2_merging_ignores_particles():
    kind, stage = "mcpe", R.stage_of("mcpe")
    r = CV.SeriesRelabeler(R.SLICE_MAP)
    for n, seed in ((6000, 3), (9000, 4)):
        _, records, series = R.random_form(kind, stage, n, seed)
        assert R.has_a_disturbed_run(kind, records, series, R.SLICE_MAP)
        new, table, _ = r.mcpe_series_host(records, series)
        for window in (0.0, 2.5):
            before = CV.MCPEGenerator.MergeHost(records, series, window)
            after = CV.MCPEGenerator.MergeHost(new, table, window)
            assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
            parents, ranges = r.parents_host(before[2], before[3])
            assert parents.tobytes() == after[2].tobytes() and ranges.tobytes() == after[3].tobytes()
            assert len(parents) < len(before[2])                        # slices of one muon in one group: duplicates were dropped


def test_p3_union_and_relabel_commute(forms):
    kind, stage, made = forms
    union = CV.MCPEGenerator.UnionHost if kind == "mcpe" else CV.FramePhotonStore.UnionHost
    (_, a, a_series), (_, b, b_series) = made[0], made[1]
    whole = union(a, a_series, b, b_series)
    assert R.has_a_disturbed_run(kind, *whole, R.SLICE_MAP) and R.has_a_disturbed_run(kind, a, a_series, R.SLICE_MAP)
    ra, rb, rw = (R.host(kind, *x, R.SLICE_MAP) for x in ((a, a_series), (b, b_series), whole))
    got = union(ra[0], ra[1], rb[0], rb[1])
    assert got[0].tobytes() == rw[0].tobytes() and got[1].tobytes() == rw[1].tobytes()


def test_p4_relabelling_twice_is_relabelling_once(forms):
    kind, stage, made = forms
    _, records, series = made[2]
    once = R.host(kind, records, series, R.SLICE_MAP)
    twice = R.host(kind, once[0], once[1], R.SLICE_MAP)
    assert twice[0].tobytes() == once[0].tobytes() and twice[2][2] == 0 and once[2][2] > 0


def test_the_parent_table():
    r = CV.SeriesRelabeler(R.relabel_map([(5, 1), (6, 1)]))
    parents = np.array([(1, 0), (1, 2), (5, 0), (5, 1), (6, 2), (9, 0), (6, 0), (7, 0)], dtype=CV.MCPE_PARENT_DTYPE)
    ranges = np.array([(0, 6), (6, 0), (6, 2)], dtype=CV.MCPE_PARENT_RANGE_DTYPE)
    got, got_ranges = r.parents_host(parents, ranges)
    assert [tuple(p) for p in got] == [(1, 0), (1, 1), (1, 2), (9, 0), (1, 0), (7, 0)]
    assert [tuple(x) for x in got_ranges] == [(0, 4), (4, 0), (4, 2)]
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception):
        r.parents_host(parents, np.array([(0, 6), (7, 1)], dtype=CV.MCPE_PARENT_RANGE_DTYPE))


@pytest.mark.parametrize("kind", R.KINDS)
def test_refusals(kind):
    records, series, m = R.run_case(kind, 4, True)
    for bad in ([(5, 1), (5, 2)], [(6, 1), (5, 2)], [(5, 6), (6, 1)], [(5, 5)]):       # not strictly ascending; a `to` among the `from`s
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as err:
            R.host(kind, records, series, R.relabel_map(bad))
        assert err.value.code == _lib.ERR_ARGUMENT
    swapped = records.copy()
    swapped[[0, 1]] = swapped[[1, 0]]                                   # no series form
    shorter = series.copy()
    shorter["count"][0] -= 1
    for r, s in ((swapped, series), (records, shorter), (records, series[:0])):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as err:
            R.host(kind, r, s, m)
        assert err.value.code == _lib.ERR_ARGUMENT
    assert _lib.load().clsimhip_series_relabel_workspace_bytes(100, 10, 24) == 0
    assert _lib.load().clsimhip_series_relabel_workspace_bytes(100, 10, 16) == _lib.load().clsimhip_series_relabel_workspace_bytes(100, 10, 48) > 0


CHECK_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "muon_slicer.h"
#include "series_relabel.h"
#include "host_model.h"
using namespace clsimhip;
template <class F> static bool refused(F f) { try { f(); } catch (const Error &e) { return e.code == CLSIMHIP_ERR_ARGUMENT; } return false; }
template <class Rec, class Fn> static int runs(Fn relabel)
{
    int bad = 0;
    for (size_t length : {size_t{1}, size_t{2}, size_t{65}, size_t{2048}, size_t{2049}, size_t{5000}})
        for (int disturbed = 0; disturbed < 2; ++disturbed) {
            std::vector<Rec> r(length), out(length);
            std::memset(r.data(), 0, length * sizeof(Rec));
            for (size_t i = 0; i < length; ++i) { r[i].identifier = i < length / 2 ? 1001u : 1005u; r[i].string_id = 1; r[i].om_id = 25; r[i].time = 20.; }
            const clsimhip_mcpe_series s{7u, 1, 25, 0u, (uint32_t)length};
            const clsimhip_relabel map[1] = {{1005u, disturbed ? 1000u : 1003u}};
            uint64_t counters[2];
            size_t kept = 0;
            relabel(r.data(), length, &s, 1, map, 1, out.data(), counters, &kept);
            const bool overflows = disturbed && length > 2048 && length >= 2;
            bad += (kept == (overflows ? 0u : length)) ? 0 : 1;
            bad += (counters[1] == (overflows ? length : 0u)) ? 0 : 1;
            for (size_t i = 1; i < kept; ++i) bad += out[i].identifier < out[i - 1].identifier ? 1 : 0;
            const clsimhip_relabel twice[2] = {{5u, 1u}, {5u, 2u}}, onward[2] = {{5u, 6u}, {6u, 1u}};
            bad += refused([&] { relabel(r.data(), length, &s, 1, twice, 2, out.data(), counters, &kept); }) ? 0 : 1;
            bad += refused([&] { relabel(r.data(), length, &s, 1, onward, 2, out.data(), counters, &kept); }) ? 0 : 1;
            bad += refused([&] { relabel(r.data(), length, &s, 0, map, 1, out.data(), counters, &kept); }) ? 0 : 1;
        }
    return bad;
}
int main()
{
    int bad = runs<clsimhip_mcpe>(mcpe_series_relabel_host) + runs<clsimhip_frame_photon>(frame_photons_relabel_host);
    // the slicer: a muon of 50 m with 40 losses, then every refusal
    std::vector<clsimhip_tree_particle> tree(41), out(128);
    std::memset(tree.data(), 0, tree.size() * sizeof(tree[0]));
    for (size_t i = 0; i < tree.size(); ++i) {
        clsimhip_tree_particle &p = tree[i];
        p.particle.type = i ? 11 : 13; p.particle.dz = 1.; p.particle.energy = i ? 1. : 100.; p.particle.length = i ? NAN : 50.;
        p.particle.z = i * 1.2; p.particle.time = i * 1.2 / 0.299792458; p.particle.identifier = 1u + (uint32_t)i; p.speed = 0.299792458; p.parent = i ? 0 : -1;
    }
    const clsimhip_mmc_track track{1u, 0u, 100., 20., 0., 50. / 0.299792458};
    std::vector<clsimhip_relabel> relabel(64);
    size_t n_out = 0, n_relabel = 0;
    uint64_t counters[5];
    slice_muons(tree.data(), tree.size(), &track, 1, 1000u, out.data(), out.size(), &n_out, relabel.data(), relabel.size(), &n_relabel, counters);
    bad += (n_out == 82 && n_relabel == 41) ? 0 : 1;
    slice_muons(tree.data(), tree.size(), &track, 1, 1000u, out.data(), 3, &n_out, relabel.data(), 2, &n_relabel, nullptr);      // short outputs
    const auto slicer_refuses = [&](std::vector<clsimhip_tree_particle> t, std::vector<clsimhip_mmc_track> k, uint32_t first) {
        return refused([&] { slice_muons(t.data(), t.size(), k.data(), k.size(), first, out.data(), out.size(), &n_out, relabel.data(), relabel.size(), &n_relabel, counters); });
    };
    std::vector<clsimhip_tree_particle> t = tree;
    t[3].particle.type = -13; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    t = tree; t[3].particle.type = 0; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    t = tree; t[0].speed = NAN; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    t = tree; t[0].particle.energy = NAN; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    t = tree; t[0].particle.time = NAN; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    t = tree; t[5].particle.time = 0.; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    t = tree; t[1].particle.time = NAN; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    t = tree; t[0].particle.energy = 0.; bad += slicer_refuses(t, {}, 1000u) ? 0 : 1;
    t = tree; t[4].parent = 4; bad += slicer_refuses(t, {track}, 1000u) ? 0 : 1;
    bad += slicer_refuses(tree, {track, track}, 1000u) ? 0 : 1;
    bad += slicer_refuses(tree, {track}, 41u) ? 0 : 1;
    bad += slicer_refuses(tree, {track}, 0xfffffff0u) ? 0 : 1;
    std::printf("host check: %d failures\n", bad);
    return bad ? 1 : 0;
}
"""


def test_host_code_under_the_sanitizers(tmp_path):
    """muon_slicer.cpp and series_relabel.cpp with a main of their own under -fsanitize=address,undefined: runs up to 2 049 and 5 000
    records, the refusals of both stages.  No Python and nothing preloaded: the program is the process."""
    clang = os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "clang++"
    src = os.path.join(ROOT, "clsim_amd", "csrc")
    main = tmp_path / "relabel_check.cpp"
    main.write_text(CHECK_MAIN)
    exe = tmp_path / "relabel_check"
    subprocess.run([clang, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + src,
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe), str(main), os.path.join(src, "muon_slicer.cpp"),
                    os.path.join(src, "series_relabel.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and "host check: 0 failures" in done.stdout, done.stdout + done.stderr
