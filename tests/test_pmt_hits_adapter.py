"""The multi-PMT hit generator through the C++ adapter (clsim_amd/cxx/pmt_adapter_test.cxx): SetPMTHitGenerator and the accessor
for the last result's hits, compiled with g++ against include/clsimhip.h and linked to libclsimhip.so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "pmt_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "pmt_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_takes_a_generator_and_refuses_a_dom_without_module(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "configured with a PMT hit generator" in out and "pmt adapter ok" in out


@pytest.mark.gpu
def test_adapter_returns_the_hits_of_its_result(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    m = re.search(r"identifier 42 photons (\d+) hits (\d+) equal to the host twin", out)
    assert m and 0 < int(m.group(2)) < int(m.group(1)), out
    assert "view: identifier 43" in out and out.rstrip().endswith("pmt adapter ok")
