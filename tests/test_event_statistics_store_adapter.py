"""The event statistics frame store through the C++ adapter (clsim_amd/cxx/I3EventStatisticsStoreHIP.h,
event_statistics_store_adapter_test.cxx): Add with the converter adapter's GetLastEventStatistics() view and a relabel map, Drain as
per-frame maps of particle -> (counts, weights); compiled with g++ against include/clsimhip.h and linked to libclsimhip.so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "event_statistics_store_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "event_statistics_store_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_host_store_folds_slices_and_gives_up_frames(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "host store: 3 bunches 9 records, 2 empty, frames <= 4 gave 2 particles in 2 frames, the rest 2 particles in one frame" in out
    assert out.rstrip().endswith("event statistics store adapter ok (no GPU run requested)")


@pytest.mark.gpu
def test_adapter_stores_every_result_of_a_converter(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    m = re.search(r"bunches 3 records 48 particles 8 head (\d+) tail (\d+) generated (\d+) at DOMs (\d+) equal to the host twin", out)
    assert m, out
    head, tail, generated, at_doms = (int(g) for g in m.groups())
    assert head == 5 and tail == 3 and generated == 3 * 1000 * 200 and 0 < at_doms < generated, out
    assert out.rstrip().endswith("event statistics store adapter ok")
