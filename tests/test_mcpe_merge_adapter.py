"""MCPE merging through the C++ adapter (clsim_amd/cxx/mcpe_merge_adapter_test.cxx): SetMCPEMerging, the flat views of the last
result and the per-frame maps (merged I3MCPESeriesMap, I3ParticleIDMap); compiled with g++ against include/clsimhip.h and linked to
libclsimhip.so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "mcpe_merge_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "mcpe_merge_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_refuses_merging_without_the_series_stage(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "configured with MCPE merging" in out and "mcpe merge adapter ok" in out


@pytest.mark.gpu
def test_adapter_returns_the_merged_series_of_its_result(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    m = re.search(r"identifier 42 photons (\d+) mcpes (\d+) series (\d+) merged (\d+) parents (\d+) frames 3 equal to the host twin", out)
    assert m, out
    photons, mcpes, series, merged, parents = (int(g) for g in m.groups())
    assert 0 < series <= merged < mcpes < photons and merged <= parents <= mcpes, out
    assert out.rstrip().endswith("mcpe merge adapter ok")
