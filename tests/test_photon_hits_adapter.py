"""Photon hits through the C++ adapter (clsim_amd/cxx/I3PhotonToMCPEConverterHIP.h, driven by photon_hits_adapter_test.cxx): the
module's parameter names build the maker, Convert() returns the host twin's records and, with MergeHits, the merging twin's; a
condition the reference ends the run on throws with its text.  Compiled with g++ against include/clsimhip.h alone and linked to
libclsimhip.so.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from clsim_amd import converter as CV
from tests import frame_photons_common as F
from tests import photon_hits_common as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("photon_hits_adapter") / "photon_hits_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "photon_hits_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def run(program, tmp_path, records, series, s, window):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    P.write_input(src, records, series, s)
    done = subprocess.run([program, src, dst, repr(float(window))], capture_output=True, text=True, timeout=120)
    return done, (open(dst, "rb").read() if done.returncode == 0 else None)


@pytest.mark.parametrize("configuration,window", [("correction_live", -1.0), ("rotated", 25.0), ("efficiencies", 0.0), ("inactive", 100.0)])
def test_adapter_returns_the_twins_records(program, tmp_path, configuration, window):
    records, series = P.synthetic_records(6000, 3)
    s = P.configuration(configuration, F.DOM_STRINGS, F.DOM_OMS)
    maker = P.maker_of(s)
    mcpes, table, counters = maker.MakeHitsHost(records, series)
    want = [mcpes, table]
    if window >= 0:
        want += list(CV.MCPEGenerator.MergeHost(mcpes, table, window))
    else:
        want += [mcpes[:0].view(CV.MCPE_MERGED_DTYPE), table[:0], np.zeros(0, CV.MCPE_PARENT_DTYPE), np.zeros(0, CV.MCPE_PARENT_RANGE_DTYPE)]
    done, out = run(program, tmp_path, records, series, s, window)
    assert done.returncode == 0 and not done.stderr, done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert lines[0] == "configured with %d DOMs" % len(s["doms"]) and lines[-1] == "photon hits adapter ok"
    assert float(lines[1].split()[-1]) == maker.Efficiency(s["doms"]["stringID"][0], s["doms"]["omID"][0])
    assert lines[2].split() == ["mcpes", str(len(want[0])), "series", str(len(want[1])), "merged", str(len(want[2])), "merged_series", str(len(want[3])),
                                "parents", str(len(want[4])), "ranges", str(len(want[5])), "inactive", str(counters["inactive"]), "off_surface", "0"]
    assert len(mcpes) > 50 and out == b"".join(w.tobytes() for w in want)
    if configuration == "inactive":
        assert counters["inactive"] > 0


def test_adapter_throws_what_the_reference_ends_on(program, tmp_path):
    records, series = P.synthetic_records(6000, 3)
    records = records.copy()
    strings, oms = F.DOM_STRINGS, F.DOM_OMS
    cases = []
    negative = records.copy()
    negative["weight"][::100] = -1.0
    cases.append((negative, series, P.configuration("check_off", strings, oms), "Photon with negative weight found. (60 photons)"))
    cases.append((records, series, P.configuration("check_on", strings, oms), "distance not DOMOversizeFactor*DOMRadiusWithoutOversize"))
    cases.append((records, series, P.spec(P.dom_table(strings[12:], oms[12:])), "OM not found in the current geometry map!"))
    cases.append((records, series, P.spec(P.dom_table(strings, oms), tables=[(2.6e-7, 1e-8, np.full(44, 3.0))]), "hitProbability > 1: your hit weights are too high."))
    cases.append((records, series[1:], P.configuration("check_off", strings, oms), "the series table does not describe the photons"))
    cases.append((records, series, P.spec(P.dom_table(strings, oms, efficiencies=(P.NAN,))), "found in the current calibration map, but it is NaN!"))
    for r, t, s, text in cases:
        done, _ = run(program, tmp_path, r, t, s, 10.0)
        assert done.returncode == 3 and ("refused: " in done.stdout and text in done.stdout), done.stdout + done.stderr
    # with OnlyWarnAboutInvalidPhotonPositions the positions are counted, not fatal
    s = P.configuration("warn_on", strings, oms)
    done, _ = run(program, tmp_path, records, series, s, -1.0)
    want = P.maker_of(s).MakeHitsHost(records, series)[2]["off_surface"]
    assert done.returncode == 0 and want > 0 and done.stdout.splitlines()[2].split()[-1] == str(want)
