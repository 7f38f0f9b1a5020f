"""Frame photons through the C++ adapter (clsim_amd/cxx/frame_photons_adapter_test.cxx): SetFramePhotons, EnqueueSteps with a particle
table and a mask, and the accessors for the last result's records, series table and per-frame maps, compiled with g++ against
include/clsimhip.h and linked to libclsimhip.so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "frame_photons_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "frame_photons_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_takes_the_switch_without_a_generator(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "configured with the frame photons stage" in out and "frame photons adapter ok" in out


@pytest.mark.gpu
def test_adapter_returns_the_series_of_its_result(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    m = re.search(r"identifier 42 photons (\d+) records (\d+) series (\d+) masked (\d+) equal to the host twin", out)
    assert m and 1 < int(m.group(3)) <= int(m.group(2)) < int(m.group(1)) and int(m.group(4)) > 0, out
    assert out.rstrip().endswith("frame photons adapter ok")
