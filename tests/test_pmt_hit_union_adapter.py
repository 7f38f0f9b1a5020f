"""The PMT hit frame store through the C++ adapter (clsim_amd/cxx/I3PMTHitFrameStoreHIP.h, pmt_hit_frame_store_adapter_test.cxx): Add
with the converter adapter's flat views, Drain as per-frame, per-module, per-PMT maps; compiled with g++ against include/clsimhip.h
and linked to libclsimhip.so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")


def build(tmp_path):
    exe = str(tmp_path / "pmt_hit_frame_store_adapter_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(CXX, "pmt_hit_frame_store_adapter_test.cxx"),
                           "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip", "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")])
    return exe


def test_adapter_host_store_takes_three_bunches_and_gives_up_frames(tmp_path):
    out = subprocess.check_output([build(tmp_path)], text=True)
    assert "host store: 3 bunches 8 hits 5 series, frames <= 4 gave 5 hits in 2 frames, the rest 3 hits on 2 PMTs of one module" in out
    assert out.rstrip().endswith("pmt hit frame store adapter ok (no GPU run requested)")


@pytest.mark.gpu
def test_adapter_stores_every_result_of_a_converter(tmp_path):
    out = subprocess.check_output([build(tmp_path), "run"], text=True)
    m = re.search(r"bunches 3 hits (\d+) series (\d+) head (\d+) tail (\d+) equal to the host twin", out)
    assert m, out
    hits, series, head, tail = (int(g) for g in m.groups())
    assert 0 < series < hits and head + tail == hits and head > 0 and tail > 0, out
    assert out.rstrip().endswith("pmt hit frame store adapter ok")
