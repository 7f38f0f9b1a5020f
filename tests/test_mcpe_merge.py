"""MCPE merging, host side: the host twin (clsimhip_mcpe_merge_host) against an independent numpy restatement of the definition,
byte for byte, on the committed fixtures' MCPEs and on synthetic series; the properties the definition promises, asserted from the
arrays alone; the edge cases, each with the groups worked out by hand; the refusals; the twin as a stand-alone program under the
sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from clsim_amd import _lib
from clsim_amd import converter as CV
from tests import mcpe_common as M
from tests import mcpe_merge_common as MM
from tests import mcpe_series_common as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
MERGE = CV.MCPEGenerator.MergeHost


def test_struct_layouts():
    assert CV.MCPE_MERGED_DTYPE.itemsize == 16 and CV.MCPE_PARENT_DTYPE.itemsize == 8 == CV.MCPE_PARENT_RANGE_DTYPE.itemsize
    assert CV.MCPE_MERGED_DTYPE.fields["time"][1] == 8 and CV.MCPE_MERGED_DTYPE.fields["stringID"][1] == 4
    header = open(os.path.join(ROOT, "include", "clsimhip.h")).read()
    assert re.search(r"sizeof\(clsimhip_mcpe_merged\) == 16 \? 1 : -1", header)
    assert "UNPINNED AGAINST THE REFERENCE" in header


@pytest.mark.parametrize("name", M.FIXTURES)
def test_twin_equals_numpy_on_the_fixtures(name):
    gen = M.standard_generator(M.pancake_of(name))
    mcpes, _ = gen.ConvertHost(M.fixture_photons(name))
    records, series, _ = gen.MakeSeriesHost(mcpes, S.particle_table(mcpes["id"]))
    assert len(records) > 0
    merged_any = False
    for window in (0.0, 5.0, 200.0, 1e9):
        got = MERGE(records, series, window)
        MM.same(got, MM.numpy_merge(records, series, window))
        MM.check_properties(records, series, window, got)
        merged_any |= len(got[0]) < len(records)
    assert len(got[0]) == len(series)               # a window longer than any series: one group each
    assert merged_any or len(series) == len(records)


def test_twin_equals_numpy_on_synthetic_series():
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(20000, seed=1)
    records, series, _ = gen.MakeSeriesHost(m, S.particle_table(m["id"]))
    assert (~np.isfinite(records["time"])).sum() >= 16 and len(set(series["frame"])) == 3
    sizes = set()
    for window in (0.0, 0.5, 3.0, 40.0, 1e4):
        got = MERGE(records, series, window)
        MM.same(got, MM.numpy_merge(records, series, window))
        MM.check_properties(records, series, window, got)
        sizes.add(len(got[0]))
        # the same identifier more than once in a group, and groups of several particles
        assert window < 3.0 or (len(got[2]) < len(records) and (got[0]["npe"] > 1).any())
    assert len(sizes) == 5
    # whole-nanosecond ties: with window 0 bit-equal times still merge
    assert len(MERGE(records, series, 0.0)[0]) < len(records)


@pytest.mark.parametrize("name", sorted(MM.edge_cases()))
def test_edge_cases(name):
    MM.check_edge_claims()
    entries, window, npe, parents = MM.edge_cases()[name]
    gen = S.synthetic_generator()
    records, series = MM.series_of(gen, MM.mcpes_of(entries))
    got = MERGE(records, series, window)
    MM.same(got, MM.numpy_merge(records, series, window))
    MM.check_properties(records, series, window, got)
    if npe is not None:
        assert got[0]["npe"].tolist() == npe
        assert list(zip(got[2]["id"].tolist(), got[2]["index"].tolist())) == parents
    if name == "special_times":
        special = ~np.isfinite(records["time"])
        assert special.sum() == 8 and (~np.isfinite(got[0]["time"])).sum() == 8            # +-inf, +-NaN, twice: every one a group of its own
        assert set(got[0]["time"][~np.isfinite(got[0]["time"])].view(np.uint64).tolist()) == set(records["time"][special].view(np.uint64).tolist())
        assert (records["time"].view(np.uint64) == 0x8000000000000000).any()
    if name == "window_zero":
        assert got[0]["time"].view(np.uint64)[0] == 0x8000000000000000                      # the opener's time: -0.0


def test_bad_arguments_are_refused():
    gen = S.synthetic_generator()
    records, series = MM.series_of(gen, MM.mcpes_of([(1, 0, 1.0), (2, 0, 2.0), (3, 1, 3.0)]))
    for window in (-1.0, -5e-324, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception) as e:
            MERGE(records, series, window)
        assert e.value.code == _lib.ERR_ARGUMENT
    assert len(MERGE(records, series, -0.0)[0]) == 3 and len(MERGE(records, series, 1.7e308)[0]) == 2
    # a table that does not partition the records
    for broken in (series[:1], series[::-1], np.concatenate([series, series[-1:]])):
        with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception, match="series table") as e:
            MERGE(records, broken, 1.0)
        assert e.value.code == _lib.ERR_ARGUMENT
    empty = series.copy()
    empty["count"] = [2, 0]
    empty["first"] = [0, 2]
    with pytest.raises(CV.I3CLSimStepToPhotonConverter_exception):
        MERGE(records[:2], empty, 1.0)


# ---- the stand-alone host program under the sanitizers ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/mcpe_merge_host_main.cpp and clsim_amd/csrc/mcpe_merge.cpp, host code only, with -fsanitize=address,undefined"""
    d = tmp_path_factory.mktemp("mcpe_merge_host_main")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "clsim_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + flags + ["-c", os.path.join(ROOT, "clsim_amd", "csrc", "mcpe_merge.cpp"),
                                                                         os.path.join(ROOT, "tests", "mcpe_merge_host_main.cpp")], cwd=str(d))
    exe = str(d / "mcpe_merge_host_main")
    # (linked without the HIP runtime: the twin makes no HIP call)
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-fsanitize=address,undefined", "mcpe_merge.o", "mcpe_merge_host_main.o", "-o", exe], cwd=str(d))
    return exe


def run_host_program(exe, tmp_path, records, series, window):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<2QdQ", len(records), len(series), window, 0))
        f.write(np.ascontiguousarray(records).tobytes())
        f.write(np.ascontiguousarray(series).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    if run.returncode != 0:
        return run, None
    blob = open(dst, "rb").read()
    n_merged, n_parents = struct.unpack_from("<2Q", blob)
    out, at = [], 16
    for count, dtype in ((n_merged, CV.MCPE_MERGED_DTYPE), (len(series), CV.MCPE_SERIES_DTYPE), (n_parents, CV.MCPE_PARENT_DTYPE),
                         (len(series), CV.MCPE_PARENT_RANGE_DTYPE)):
        out.append(np.frombuffer(blob, dtype=dtype, count=count, offset=at))
        at += count * dtype.itemsize
    assert at == len(blob)
    return run, tuple(out)


def test_host_program_runs_clean_under_the_sanitizers(host_program, tmp_path):
    gen = S.synthetic_generator()
    m = S.synthetic_mcpes(5000, seed=4)
    records, series, _ = gen.MakeSeriesHost(m, S.particle_table(m["id"]))
    inputs = [(records, series, 0.0), (records, series, 25.0), (records[:0], series[:0], 1.0)]
    for name in ("special_times", "overflow", "one_record", "many_particles_one_group"):
        entries, window, _, _ = MM.edge_cases()[name]
        inputs.append(MM.series_of(gen, MM.mcpes_of(entries)) + (window,))
    for r, s, window in inputs:
        run, out = run_host_program(host_program, tmp_path, r, s, window)
        assert run.returncode == 0 and run.stderr == "", run.stderr
        MM.same(out, MERGE(r, s, window))
    run, _ = run_host_program(host_program, tmp_path, records, series, float("nan"))
    assert run.returncode == 3 and "refused" in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr
