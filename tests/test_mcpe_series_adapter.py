"""The MCPE series through the C++ adapter (clsim_amd/cxx/mcpe_series_adapter_test.cxx): SetMCPESeries, EnqueueSteps with a particle
table and ignored modules, the flat views and the per-frame maps of the last result; compiled with g++ against include/clsimhip.h
and linked to libclsimhip.so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "mcpe_series_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "mcpe_series_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_refuses_series_without_a_generator(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "configured with MCPE series" in out and "mcpe series adapter ok" in out


@pytest.mark.gpu
def test_adapter_returns_the_series_of_its_result(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    m = re.search(r"identifier 42 photons (\d+) mcpes (\d+) series (\d+) frames 3 masked (\d+) equal to the host twin", out)
    assert m and 0 < int(m.group(3)) <= int(m.group(2)) < int(m.group(1)) and int(m.group(4)) > 0, out
    assert out.rstrip().endswith("mcpe series adapter ok")
