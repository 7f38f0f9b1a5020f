"""Event statistics through the C++ adapter (clsim_amd/cxx/event_statistics_adapter_test.cxx): SetEventStatistics and the accessors
for the last result's records and counters, compiled with g++ against include/clsimhip.h and the adapter's stand-ins for the
framework's types, and linked to libclsimhip.so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "event_statistics_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "event_statistics_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_takes_the_switch_and_the_helpers_add_and_round(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "configured with the event statistics stage" in out and "event statistics adapter ok" in out


@pytest.mark.gpu
def test_adapter_returns_the_records_of_its_result(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    m = re.search(r"identifier 42 photons (\d+) at DOMs (\d+) masked (\d+) equal to the host twin", out)
    assert m and 0 < int(m.group(2)) and 0 < int(m.group(3)) and int(m.group(2)) + int(m.group(3)) == int(m.group(1)), out
    assert out.rstrip().endswith("event statistics adapter ok")
