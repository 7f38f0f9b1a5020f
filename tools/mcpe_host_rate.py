#!/usr/bin/env python3
"""Single-thread rate of the MCPE generator's host twin (clsimhip_mcpe_convert_host), in photon records per second.
No GPU: the committed photon records of tests/golden/verbatim_cl_*.npz, repeated to `--records` records, best of `--repeats`.

    python tools/mcpe_host_rate.py [--records 2000000] [--repeats 5]

--series N: the MCPE series' host twin instead (clsimhip_mcpe_series_host: lookup, mask, shift, sort, series table), in MCPEs per
second, on N synthetic MCPEs at IceCube's 5160 DOMs dealt to 1000 particles in 10 frames; --device adds the device stage's time
for the same input (HIP events around clsimhip_mcpe_series_device, best of --repeats; needs a GPU).

--merge: the MCPE merging host twin instead (clsimhip_mcpe_merge_host), in records per second, on one DOM with 130 000 records of 7
particles as a long chain of groups (window 5 ns) and as one group, and on 300 000 synthetic records in 420 series (window 2 ns);
--device adds the device stage's time for the same inputs (HIP events around clsimhip_mcpe_merge_device; needs a GPU).

--union N M: the MCPE frame store's union instead (clsimhip_mcpe_series_union_host, one thread), in records per second: a store of the
series of N synthetic MCPEs meets a bunch of the series of M more, at IceCube's 5160 DOMs dealt to 1000 particles in 10 frames;
--one-dom puts every record on one DOM of one frame (one series across all output tiles).  --device adds the union kernels' time for
the same input (HIP events around clsimhip_mcpe_series_union_device, best of --repeats; needs a GPU) and, as the yardstick, the
series stage re-sorting the N + M MCPEs (clsimhip_mcpe_series_device) in the same run.

--frame-photon-union N M: the frame photon store's union instead (clsimhip_frame_photons_union_host, one thread), in records per
second: a store of the frame photons of N synthetic photon records meets a bunch of the frame photons of M more, at 5160 DOMs dealt
to 1000 particles in 10 frames; --one-dom puts every record on one module of one frame.  --device adds the union kernels' time for the
same input (HIP events around clsimhip_frame_photons_union_device, best of --repeats; needs a GPU) and, as the yardstick, the frame
photons stage re-sorting the N + M source photons (clsimhip_frame_photons_device) in the same run.

--pmt-hit-union N M: the PMT hit frame store's union instead (clsimhip_pmt_hits_union_host, one thread), in records per second: a
store of the PMT series of N synthetic hits meets a bunch of the PMT series of M more, at 5160 modules of 31 PMTs dealt to 1000
particles in 10 frames; --one-channel puts every record on one PMT of one module of one frame (one series across all output tiles).
--device adds the union kernels' time for the same input (HIP events around clsimhip_pmt_hits_union_device, best of --repeats; needs
a GPU) and, as the yardstick, the PMT series stage re-sorting the N + M hits (clsimhip_pmt_series_device) in the same run.

--pmt: the multi-PMT hit generator's host twin instead (clsimhip_pmt_convert_host) on the same records, against the 31-PMT layout
of tests/pmt_common.py, in photon records per second.

--pmt-series N: the PMT series' host twin instead (clsimhip_pmt_series_host), in hits per second, on N synthetic hits at 5160
modules of 31 PMTs dealt to 1000 particles in 10 frames; --device adds the device stage's time for the same input (HIP events
around clsimhip_pmt_series_device, best of --repeats; needs a GPU).

--frame-photons N: the frame photons' host twin instead (clsimhip_frame_photons_host), in photon records per second, on N synthetic
records at 5160 DOMs dealt to 1000 particles in 10 frames; --device likewise (clsimhip_frame_photons_device).

--cable-shadow N: the cable shadow's host twin instead (clsimhip_cable_shadow_host), in photon records and in segment-cylinder tests
per second, on N records against --cylinders cylinders (default 5160: one cable beside every DOM of an 86 x 60 detector, in detector
coordinates like the reference's I3CylinderMap, so that a record can only meet the cable of its own DOM and walks the whole set
otherwise); --device adds the device stage's time for the same input (HIP events around clsimhip_cable_shadow_device, best of
--repeats; needs a GPU) -- the host twin then runs once, for the comparison.

--event-statistics N: the event statistics' host twin instead (clsimhip_event_statistics_host), in records per second, on N steps and
N photon records dealt to 1000 particles in 10 frames in runs of 4096 (a particle's steps and photons come in long runs), weights
over twelve binades; --device adds the device stage's time for the same input (HIP events around clsimhip_event_statistics_device,
best of --repeats; needs a GPU).

--photon-hits N: the photon hits' host twin instead (clsimhip_photon_hits_host), in frame photon records per second, on the committed
photon records repeated to N records, dealt to 5160 DOMs and 1000 particles in 10 frames and brought into form by the frame photons'
host twin; IceCube acceptance, efficiencies from {0.5, 1, 1.35}, pancake 2 of oversize 5 (the time correction is live); --device adds
the device stage's time for the same input (HIP events around clsimhip_photon_hits_device, best of --repeats; needs a GPU).  The line
names the core the host twin ran on.

--pmt-photon-hits N: the PMT photon hits' host twin instead (clsimhip_pmt_photon_hits_host), on the same input as --photon-hits, with a
31-PMT module (tests/pmt_common.py) at every one of the 5160 DOMs; --device adds the device stage's time for the same input (HIP
events around clsimhip_pmt_photon_hits_device, best of --repeats; needs a GPU).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clsim_amd import _lib                      # noqa: E402
from clsim_amd import converter as CV           # noqa: E402
from tests import mcpe_common as M              # noqa: E402


def series_rate(args):
    n = args.series
    rng = np.random.default_rng(1)
    s, d = np.meshgrid(np.arange(1, 87), np.arange(1, 61), indexing="ij")
    s, d = s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)
    gen = M.make_generator([M.acceptance_table()], s, d, np.zeros(len(s), dtype=np.int32))
    m = np.zeros(n, dtype=CV.MCPE_DTYPE)
    dom = rng.integers(0, len(s), n)
    m["stringID"], m["omID"], m["id"], m["time"] = s[dom], d[dom], rng.integers(0, 1000, n), rng.uniform(0.0, 1.0e4, n)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, rng.uniform(0.0, 1.0e6, 1000)
    masked = np.zeros(20, dtype=CV.MCPE_MASK_DTYPE)
    masked["frame"], masked["stringID"], masked["omID"] = np.arange(20) % 10, 40, 30
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        records, series, counters = gen.MakeSeriesHost(m, p, masked)
        best = min(best, time.perf_counter() - t0)
    line = {"mcpes": n, "kept": len(records), "series": len(series), "host_seconds": best, "host_mcpes_per_s": n / best, "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(m.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        d_out, d_series = torch.zeros((n, 16), dtype=torch.uint8, device=dev), torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(5, dtype=torch.int32, device=dev)
        ws = CV.MCPEGenerator.SeriesWorkspaceBytes(n, len(p), len(masked))
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), n, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws,
                                 p, masked, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        got = d_out.cpu().numpy()[:len(records)].copy().view(CV.MCPE_DTYPE).reshape(-1)
        assert int(d_counts[0]) == len(records) and got.tobytes() == records.tobytes()
        line.update(device_seconds=min(times[1:]), device_mcpes_per_s=n / min(times[1:]))
    print(json.dumps(line))


def pmt_series_rate(args):
    from tests import pmt_common as PC
    n = args.pmt_series
    rng = np.random.default_rng(1)
    s, d = np.meshgrid(np.arange(1, 87), np.arange(1, 61), indexing="ij")
    s, d = s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)
    types, pmts = PC.layout(PC.sphere_radius_of("mie"))
    modules = np.zeros(len(s), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"], modules["rotation"] = s, d, np.eye(3).reshape(9)
    gen = PC.make_generator(PC.standard_functions(), types, pmts, modules)
    h = np.zeros(n, dtype=CV.PMT_HIT_DTYPE)
    at = rng.integers(0, len(s), n)
    h["stringID"], h["omID"], h["pmt"], h["id"], h["time"] = s[at], d[at], rng.integers(0, 31, n), rng.integers(0, 1000, n), rng.uniform(0.0, 1.0e4, n)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, rng.uniform(0.0, 1.0e6, 1000)
    masked = np.zeros(20, dtype=CV.MCPE_MASK_DTYPE)
    masked["frame"], masked["stringID"], masked["omID"] = np.arange(20) % 10, 40, 30
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        records, series, counters = gen.MakeSeriesHost(h, p, masked)
        best = min(best, time.perf_counter() - t0)
    line = {"pmt_hits": n, "kept": len(records), "series": len(series), "host_seconds": best, "host_hits_per_s": n / best, "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(h.view(np.uint8).reshape(-1, 24).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        d_out, d_series = torch.zeros((n, 24), dtype=torch.uint8, device=dev), torch.zeros((n, 24), dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(5, dtype=torch.int32, device=dev)
        ws = CV.PMTHitGenerator.SeriesWorkspaceBytes(n, len(p), len(masked))
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), n, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws,
                                 p, masked, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        got = d_out.cpu().numpy()[:len(records)].copy().view(CV.PMT_HIT_DTYPE).reshape(-1)
        assert int(d_counts[0]) == len(records) and got.tobytes() == records.tobytes()
        line.update(device_seconds=min(times[1:]), device_hits_per_s=n / min(times[1:]))
    print(json.dumps(line))


def frame_photons_rate(args):
    n = args.frame_photons
    rng = np.random.default_rng(1)
    s, d = np.meshgrid(np.arange(1, 87), np.arange(1, 61), indexing="ij")
    s, d = s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)
    doms = CV.FramePhotonDoms(s, d)
    m = np.zeros(n, dtype=CV.PHOTON_DTYPE)
    at = rng.integers(0, len(s), n)
    m["stringID"], m["omID"], m["id"], m["t"] = s[at], d[at], rng.integers(0, 1000, n), rng.uniform(0.0, 1.0e4, n)
    for name in ("x", "y", "z", "theta", "phi", "wavelength", "weight", "groupVelocity"):
        m[name] = rng.uniform(0.1, 1.0, n)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, rng.uniform(0.0, 1.0e6, 1000)
    masked = np.zeros(20, dtype=CV.MCPE_MASK_DTYPE)
    masked["frame"], masked["stringID"], masked["omID"] = np.arange(20) % 10, 40, 30
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        records, series, counters = doms.MakeFramePhotonsHost(m, p, masked)
        best = min(best, time.perf_counter() - t0)
    line = {"photon_records": n, "kept": len(records), "series": len(series), "host_seconds": best, "host_records_per_s": n / best, "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(m.view(np.uint8).reshape(-1, 80).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        d_out, d_series = torch.zeros((n, 48), dtype=torch.uint8, device=dev), torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(6, dtype=torch.int32, device=dev)
        ws = CV.FramePhotonDoms.WorkspaceBytes(n, len(p), len(masked))
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            doms.MakeFramePhotonsDevice(d_in.data_ptr(), d_cnt.data_ptr(), n, d_out.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws,
                                        p, masked, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        got = d_out.cpu().numpy()[:len(records)].copy().view(CV.FRAME_PHOTON_DTYPE).reshape(-1)
        assert int(d_counts[0]) == len(records) and got.tobytes() == records.tobytes()
        line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]))
    print(json.dumps(line))


def cable_shadow_rate(args):
    n, c = args.cable_shadow, args.cylinders
    rng = np.random.default_rng(1)
    # an 86 x 60 detector: strings 125 m apart on a square grid, DOMs 17 m apart; the cable 20 cm beside its DOM, 1 m long, 2.3 cm thick
    k = np.arange(c)
    dom = np.stack([125.0 * ((k // 60) % 10) - 560.0, 125.0 * ((k // 60) // 10) - 500.0, 500.0 - 17.0 * (k % 60)], axis=1)
    azimuth = rng.uniform(0.0, 2.0 * np.pi, c)
    beside = dom + 0.2 * np.stack([np.cos(azimuth), np.sin(azimuth), np.zeros(c)], axis=1)
    shadow = CV.CableShadow(beside + [0.0, 0.0, 0.5], beside - [0.0, 0.0, 0.5], 0.023, 1.0)
    base = np.concatenate([M.fixture_photons(name) for name in M.FIXTURES if name != "lea_no_pancake"])
    m = np.ascontiguousarray(np.tile(base, -(-n // len(base)))[:n])
    at = rng.integers(0, c, n)
    for i, name in enumerate("xyz"):            # the record's position on its DOM's sphere, in detector coordinates
        m[name] = (m[name].astype(np.float64) + dom[at, i]).astype(np.float32)
    best = float("inf")
    for _ in range(1 if args.device else args.repeats):
        t0 = time.perf_counter()
        flags, lit, counts = shadow.MakeHost(m)
        best = min(best, time.perf_counter() - t0)
    tests = float(n) * c            # (an upper bound: a shadowed record stops at its cylinder)
    line = {"photon_records": n, "cylinders": c, "shadowed": counts["shadowed"], "host_seconds": best, "host_records_per_s": n / best,
            "host_ns_per_test": best / tests * 1e9, "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(m.view(np.uint8).reshape(-1, 80).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        d_flags, d_lit = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, 80), dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(4, dtype=torch.int32, device=dev)
        ws = CV.CableShadow.WorkspaceBytes(n)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            shadow.MakeDevice(d_in.data_ptr(), d_cnt.data_ptr(), n, d_flags.data_ptr(), d_lit.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert [int(v) for v in d_counts.cpu()[:3]] == [len(lit), n, counts["shadowed"]]
        assert d_flags.cpu().numpy().tobytes() == flags.tobytes() and d_lit.cpu().numpy()[:len(lit)].tobytes() == lit.tobytes()
        line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]), device_ns_per_test=min(times[1:]) / tests * 1e9)
    print(json.dumps(line))


def event_statistics_rate(args):
    n = args.event_statistics
    rng = np.random.default_rng(1)
    ident = (np.arange(n) // 4096) % 1000
    steps = np.zeros(n, dtype=CV.STEP_DTYPE)
    steps["num"], steps["weight"], steps["id"] = rng.integers(0, 400, n), np.exp(rng.uniform(-4.0, 4.0, n)), ident
    photons = np.zeros(n, dtype=CV.PHOTON_DTYPE)
    photons["weight"], photons["id"] = np.exp(rng.uniform(-4.0, 4.0, n)), ident
    photons["stringID"], photons["omID"] = rng.integers(1, 87, n), rng.integers(1, 61, n)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"] = np.arange(1000), np.arange(1000) % 10
    masked = np.zeros(20, dtype=CV.MCPE_MASK_DTYPE)
    masked["frame"], masked["stringID"], masked["omID"] = np.arange(20) % 10, 40, 30
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        want, counters = CV.EventStatistics.MakeHost(steps, photons, p, masked)
        best = min(best, time.perf_counter() - t0)
    line = {"steps": n, "photon_records": n, "particles": len(p), "masked": counters["masked"], "host_seconds": best, "host_records_per_s": 2 * n / best,
            "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        d_steps = torch.from_numpy(steps.view(np.uint8).reshape(-1, 48).copy()).to(dev)
        d_photons = torch.from_numpy(photons.view(np.uint8).reshape(-1, 80).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        d_out = torch.zeros((len(p), 144), dtype=torch.uint8, device=dev)
        d_counters = torch.zeros(4, dtype=torch.int32, device=dev)
        ws = CV.EventStatistics.WorkspaceBytes(len(p), len(masked))
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            CV.EventStatistics.MakeDevice(d_steps.data_ptr(), n, d_photons.data_ptr(), d_cnt.data_ptr(), n, d_out.data_ptr(), d_counters.data_ptr(), d_ws.data_ptr(), ws,
                                          particles=p, masked=masked, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert d_out.cpu().numpy().tobytes() == want.tobytes() and [int(v) for v in d_counters.cpu()[:3]] == [counters[k] for k in CV.EVENT_STATISTICS_COUNTERS]
        line.update(device_seconds=min(times[1:]), device_records_per_s=2 * n / min(times[1:]))
    print(json.dumps(line))


def stored_photons(n):
    """(records, series, string IDs, OM IDs): the committed photon records repeated to n, dealt to 5160 DOMs and 1000 particles in 10 frames"""
    rng = np.random.default_rng(1)
    s, d = np.meshgrid(np.arange(1, 87), np.arange(1, 61), indexing="ij")
    s, d = s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)
    base = np.concatenate([M.fixture_photons(name) for name in M.FIXTURES if name != "lea_no_pancake"])
    m = np.ascontiguousarray(np.tile(base, -(-n // len(base)))[:n])
    at = rng.integers(0, len(s), n)
    m["stringID"], m["omID"], m["id"] = s[at], d[at], rng.integers(0, 1000, n)
    m["t"] = (m["t"] + rng.uniform(0.0, 1.0e4, n)).astype(np.float32)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, rng.uniform(0.0, 1.0e6, 1000)
    records, series, _ = CV.FramePhotonDoms(s, d).MakeFramePhotonsHost(m, p)
    return records, series, s, d


def pmt_photon_hits_rate(args):
    from tests import pmt_common as PC
    n = args.pmt_photon_hits
    records, series, s, d = stored_photons(n)
    types, pmts = PC.layout(PC.sphere_radius_of("mie"))
    modules = np.zeros(len(s), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"], modules["rotation"] = s, d, PC.IDENTITY.reshape(9)
    gen = PC.make_generator(PC.standard_functions(), types, pmts, modules)
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        hits, table, counters = gen.MakeHitsFromFramePhotonsHost(records, series)
        best = min(best, time.perf_counter() - t0)
    assert not any(counters.values())
    model = [line.split(":", 1)[1].strip() for line in open("/proc/cpuinfo") if line.startswith("model name")][:1]
    line = {"frame_photons": n, "input_series": len(series), "modules": len(modules), "pmts_per_module": 31, "pmt_hits": len(hits), "series": len(table),
            "host_seconds": best, "host_records_per_s": n / best, "threads": 1, "host_core": model[0] if model else None}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        d_records = torch.from_numpy(records.view(np.uint8).copy()).to(dev)
        d_series = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_series[:len(series) * 16] = torch.from_numpy(series.view(np.uint8).copy()).to(dev)
        d_in = torch.tensor([n, len(series)], dtype=torch.int32, device=dev)
        d_out, d_out_series = torch.zeros(n * 24, dtype=torch.uint8, device=dev), torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(7, dtype=torch.int32, device=dev)
        ws = CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(n)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            gen.MakeHitsFromFramePhotonsDevice(d_records.data_ptr(), d_series.data_ptr(), d_in.data_ptr(), n, d_out.data_ptr(), d_out_series.data_ptr(),
                                               d_counts.data_ptr(), d_ws.data_ptr(), ws, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert [int(c) for c in d_counts.cpu()[:2]] == [len(hits), len(table)]
        assert d_out.cpu().numpy()[:len(hits) * 24].tobytes() == hits.tobytes() and d_out_series.cpu().numpy()[:len(table) * 24].tobytes() == table.tobytes()
        line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]))
    print(json.dumps(line))


def photon_hits_rate(args):
    from tests import photon_hits_common as P
    n = args.photon_hits
    records, series, s, d = stored_photons(n)
    maker = P.maker_of(P.spec(P.dom_table(s, d, efficiencies=(0.5, 1.0, 1.35), spe=1.0), pancake=2.0))
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        mcpes, table, counters = maker.MakeHitsHost(records, series)
        best = min(best, time.perf_counter() - t0)
    assert not any(counters.values())
    model = [line.split(":", 1)[1].strip() for line in open("/proc/cpuinfo") if line.startswith("model name")][:1]
    line = {"frame_photons": n, "input_series": len(series), "mcpes": len(mcpes), "series": len(table), "host_seconds": best, "host_records_per_s": n / best,
            "threads": 1, "host_core": model[0] if model else None}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        d_records = torch.from_numpy(records.view(np.uint8).copy()).to(dev)
        d_series = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_series[:len(series) * 16] = torch.from_numpy(series.view(np.uint8).copy()).to(dev)
        d_in = torch.tensor([n, len(series)], dtype=torch.int32, device=dev)
        d_out, d_out_series = torch.zeros(n * 16, dtype=torch.uint8, device=dev), torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(9, dtype=torch.int32, device=dev)
        ws = CV.PhotonHitMaker.WorkspaceBytes(n)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            maker.MakeHitsDevice(d_records.data_ptr(), d_series.data_ptr(), d_in.data_ptr(), n, d_out.data_ptr(), d_out_series.data_ptr(), d_counts.data_ptr(),
                                 d_ws.data_ptr(), ws, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert [int(c) for c in d_counts.cpu()[:2]] == [len(mcpes), len(table)]
        assert d_out.cpu().numpy()[:len(mcpes) * 16].tobytes() == mcpes.tobytes() and d_out_series.cpu().numpy()[:len(table) * 16].tobytes() == table.tobytes()
        line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]))
    print(json.dumps(line))


def union_rate(args):
    n_a, n_b = args.union
    n = n_a + n_b
    rng = np.random.default_rng(1)
    s, d = np.meshgrid(np.arange(1, 87), np.arange(1, 61), indexing="ij")
    s, d = s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)
    gen = M.make_generator([M.acceptance_table()], s, d, np.zeros(len(s), dtype=np.int32))
    m = np.zeros(n, dtype=CV.MCPE_DTYPE)
    dom = rng.integers(0, len(s), n)
    m["stringID"], m["omID"], m["id"], m["time"] = s[dom], d[dom], rng.integers(0, 1000, n), rng.uniform(0.0, 1.0e4, n)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, rng.uniform(0.0, 1.0e6, 1000)
    if args.one_dom:
        m["stringID"], m["omID"], p["frame"] = 40, 30, 4
    a, b, whole = (gen.MakeSeriesHost(part, p)[:2] for part in (m[:n_a], m[n_a:], m))
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        records, series = CV.MCPEGenerator.UnionHost(*a, *b)
        best = min(best, time.perf_counter() - t0)
    assert records.tobytes() == whole[0].tobytes() and series.tobytes() == whole[1].tobytes()
    line = {"input": "one_dom" if args.one_dom else "synthetic", "store_records": n_a, "bunch_records": n_b, "series": len(series), "host_seconds": best,
            "host_records_per_s": n / best, "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev) if len(x) else torch.zeros(16, dtype=torch.uint8, device=dev)
        d_a, d_b = (up(a[0]), up(a[1]), torch.tensor([n_a, len(a[1]), 0, 0, 0], dtype=torch.int32, device=dev)), \
                   (up(b[0]), up(b[1]), torch.tensor([n_b, len(b[1]), 0, 0, 0], dtype=torch.int32, device=dev))
        d_out, d_table = torch.zeros((max(n, 1), 16), dtype=torch.uint8, device=dev), torch.zeros((max(n, 1), 16), dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(5, dtype=torch.int32, device=dev)
        # (the tables are as long as they are: the capacity of a table is that of its records, so the buffers are padded)
        pad = lambda t, entries: torch.cat([t, torch.zeros(max(entries, 1) * 16 - len(t), dtype=torch.uint8, device=dev)])
        d_a, d_b = (d_a[0], pad(d_a[1], n_a), d_a[2]), (d_b[0], pad(d_b[1], n_b), d_b[2])
        ws = CV.MCPEGenerator.UnionWorkspaceBytes(n_a, n_b)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            CV.MCPEGenerator.UnionDevice(d_a[0].data_ptr(), d_a[1].data_ptr(), d_a[2].data_ptr(), n_a, d_b[0].data_ptr(), d_b[1].data_ptr(), d_b[2].data_ptr(), n_b,
                                         d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), n, d_ws.data_ptr(), ws, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert [int(c) for c in d_counts.cpu()] == [n, len(series), 0, 0, 0]
        assert d_out.cpu().numpy().reshape(-1)[:n * 16].tobytes() == records.tobytes() and d_table.cpu().numpy().reshape(-1)[:len(series) * 16].tobytes() == series.tobytes()
        line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]))
        # the yardstick: the series stage on the N + M MCPEs
        d_in = torch.from_numpy(m.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        ws = CV.MCPEGenerator.SeriesWorkspaceBytes(n, len(p), 0)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), n, d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws, p, None, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert int(d_counts[0]) == n and d_out.cpu().numpy().reshape(-1)[:n * 16].tobytes() == records.tobytes()
        line.update(resort_device_seconds=min(times[1:]), union_over_resort=line["device_seconds"] / min(times[1:]))
    print(json.dumps(line))


def frame_photon_union_rate(args):
    n_a, n_b = args.frame_photon_union
    n = n_a + n_b
    rng = np.random.default_rng(1)
    s, d = np.meshgrid(np.arange(1, 87), np.arange(1, 61), indexing="ij")
    s, d = s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)
    doms = CV.FramePhotonDoms(s, d)
    m = np.zeros(n, dtype=CV.PHOTON_DTYPE)
    at = rng.integers(0, len(s), n)
    m["stringID"], m["omID"], m["id"], m["t"] = s[at], d[at], rng.integers(0, 1000, n), rng.uniform(0.0, 1.0e4, n)
    for name in ("x", "y", "z", "theta", "phi", "wavelength", "weight", "groupVelocity"):
        m[name] = rng.uniform(0.1, 1.0, n)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, rng.uniform(0.0, 1.0e6, 1000)
    if args.one_dom:
        m["stringID"], m["omID"], p["frame"] = 40, 30, 4
    a, b, whole = (doms.MakeFramePhotonsHost(part, p)[:2] for part in (m[:n_a], m[n_a:], m))
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        records, series = CV.FramePhotonStore.UnionHost(*a, *b)
        best = min(best, time.perf_counter() - t0)
    assert records.tobytes() == whole[0].tobytes() and series.tobytes() == whole[1].tobytes()
    line = {"input": "one_dom" if args.one_dom else "synthetic", "store_records": n_a, "bunch_records": n_b, "series": len(series), "host_seconds": best,
            "host_records_per_s": n / best, "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)

        def up(form, capacity):          # (the capacity of a table is that of its records: both buffers are padded to it)
            out = []
            for x, size in zip(form, (48, 16)):
                t = torch.zeros(max(capacity, 1) * size, dtype=torch.uint8, device=dev)
                if len(x):
                    t[:len(x) * size] = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev)
                out.append(t)
            return out + [torch.tensor([len(form[0]), len(form[1]), 0, 0, 0], dtype=torch.int32, device=dev)]
        d_a, d_b = up(a, n_a), up(b, n_b)
        d_out, d_table = torch.zeros((max(n, 1), 48), dtype=torch.uint8, device=dev), torch.zeros((max(n, 1), 16), dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(6, dtype=torch.int32, device=dev)
        ws = CV.FramePhotonStore.UnionWorkspaceBytes(n_a, n_b)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            CV.FramePhotonStore.UnionDevice(d_a[0].data_ptr(), d_a[1].data_ptr(), d_a[2].data_ptr(), n_a, d_b[0].data_ptr(), d_b[1].data_ptr(), d_b[2].data_ptr(), n_b,
                                            d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), n, d_ws.data_ptr(), ws, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert [int(c) for c in d_counts.cpu()[:5]] == [n, len(series), 0, 0, 0]
        assert d_out.cpu().numpy().reshape(-1)[:n * 48].tobytes() == records.tobytes() and d_table.cpu().numpy().reshape(-1)[:len(series) * 16].tobytes() == series.tobytes()
        line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]))
        # the yardstick: the frame photons stage re-sorting the N + M source photons
        d_in = torch.from_numpy(m.view(np.uint8).reshape(-1, 80).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        ws = CV.FramePhotonDoms.WorkspaceBytes(n, len(p), 0)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            doms.MakeFramePhotonsDevice(d_in.data_ptr(), d_cnt.data_ptr(), n, d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws, p, None,
                                        stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert int(d_counts[0]) == n and d_out.cpu().numpy().reshape(-1)[:n * 48].tobytes() == records.tobytes()
        line.update(resort_device_seconds=min(times[1:]), union_over_resort=line["device_seconds"] / min(times[1:]))
    print(json.dumps(line))


def pmt_hit_union_rate(args):
    from tests import pmt_common as PC
    n_a, n_b = args.pmt_hit_union
    n = n_a + n_b
    rng = np.random.default_rng(1)
    s, d = np.meshgrid(np.arange(1, 87), np.arange(1, 61), indexing="ij")
    s, d = s.reshape(-1).astype(np.int32), d.reshape(-1).astype(np.uint32)
    types, pmts = PC.layout(PC.sphere_radius_of("mie"))
    modules = np.zeros(len(s), dtype=CV.PMT_MODULE_DTYPE)
    modules["stringID"], modules["omID"], modules["rotation"] = s, d, np.eye(3).reshape(9)
    gen = PC.make_generator(PC.standard_functions(), types, pmts, modules)
    h = np.zeros(n, dtype=CV.PMT_HIT_DTYPE)
    at = rng.integers(0, len(s), n)
    h["stringID"], h["omID"], h["pmt"], h["id"], h["time"] = s[at], d[at], rng.integers(0, 31, n), rng.integers(0, 1000, n), rng.uniform(0.0, 1.0e4, n)
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, rng.uniform(0.0, 1.0e6, 1000)
    if args.one_channel:
        h["stringID"], h["omID"], h["pmt"], p["frame"] = 40, 30, 17, 4
    a, b, whole = (gen.MakeSeriesHost(part, p)[:2] for part in (h[:n_a], h[n_a:], h))
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        records, series = CV.PMTHitFrameStore.UnionHost(*a, *b)
        best = min(best, time.perf_counter() - t0)
    assert records.tobytes() == whole[0].tobytes() and series.tobytes() == whole[1].tobytes()
    line = {"input": "one_channel" if args.one_channel else "synthetic", "store_records": n_a, "bunch_records": n_b, "series": len(series), "host_seconds": best,
            "host_records_per_s": n / best, "threads": 1}
    if args.device:
        import torch
        dev = torch.device("cuda", 0)

        def up(form, capacity):          # (the capacity of a table is that of its records: both buffers are padded to it)
            out = []
            for x in form:
                t = torch.zeros(max(capacity, 1) * 24, dtype=torch.uint8, device=dev)
                if len(x):
                    t[:len(x) * 24] = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev)
                out.append(t)
            return out + [torch.tensor([len(form[0]), len(form[1]), 0, 0, 0], dtype=torch.int32, device=dev)]
        d_a, d_b = up(a, n_a), up(b, n_b)
        d_out, d_table = torch.zeros((max(n, 1), 24), dtype=torch.uint8, device=dev), torch.zeros((max(n, 1), 24), dtype=torch.uint8, device=dev)
        d_counts = torch.zeros(5, dtype=torch.int32, device=dev)
        ws = CV.PMTHitFrameStore.UnionWorkspaceBytes(n_a, n_b)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            CV.PMTHitFrameStore.UnionDevice(d_a[0].data_ptr(), d_a[1].data_ptr(), d_a[2].data_ptr(), n_a, d_b[0].data_ptr(), d_b[1].data_ptr(), d_b[2].data_ptr(), n_b,
                                            d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), n, d_ws.data_ptr(), ws, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert [int(c) for c in d_counts.cpu()] == [n, len(series), 0, 0, 0]
        assert d_out.cpu().numpy().reshape(-1)[:n * 24].tobytes() == records.tobytes() and d_table.cpu().numpy().reshape(-1)[:len(series) * 24].tobytes() == series.tobytes()
        line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]))
        # the yardstick: the PMT series stage re-sorting the N + M hits
        d_in = torch.from_numpy(h.view(np.uint8).reshape(-1, 24).copy()).to(dev)
        d_cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        ws = CV.PMTHitGenerator.SeriesWorkspaceBytes(n, len(p), 0)
        d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        times = []
        for _ in range(args.repeats + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            gen.MakeSeriesDevice(d_in.data_ptr(), d_cnt.data_ptr(), n, d_out.data_ptr(), d_table.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws, p, None, stream=stream)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) * 1e-3)
        assert int(d_counts[0]) == n and d_out.cpu().numpy().reshape(-1)[:n * 24].tobytes() == records.tobytes()
        line.update(resort_device_seconds=min(times[1:]), union_over_resort=line["device_seconds"] / min(times[1:]))
    print(json.dumps(line))


def merge_rate(args):
    from tests import mcpe_merge_common as MM
    from tests import mcpe_series_common as S
    gen = S.synthetic_generator()
    dom = MM.series_of(gen, MM.one_dom(130000, seed=3))
    m = S.synthetic_mcpes(300000, seed=9, n_identifiers=3000)
    many = gen.MakeSeriesHost(m, S.particle_table(m["id"], frames=(50, 10, 40, 20, 30)))[:2]
    for name, (records, series), window in (("one_dom_long_chain", dom, 5.0), ("one_dom_one_group", dom, 2e6), ("synthetic_300000", many, 2.0)):
        best = float("inf")
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            want = CV.MCPEGenerator.MergeHost(records, series, window)
            best = min(best, time.perf_counter() - t0)
        n = len(records)
        line = {"input": name, "records": n, "series": len(series), "window": window, "merged": len(want[0]), "parents": len(want[2]),
                "host_seconds": best, "host_records_per_s": n / best, "threads": 1}
        if args.device:
            import torch
            dev = torch.device("cuda", 0)
            d_records = torch.from_numpy(records.view(np.uint8).copy()).to(dev)
            d_series = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            d_series[:len(series) * 16] = torch.from_numpy(series.view(np.uint8).copy()).to(dev)
            d_series_counts = torch.tensor([n, len(series), 0, 0, 0], dtype=torch.int32, device=dev)
            outs = [torch.zeros(n * size, dtype=torch.uint8, device=dev) for size in (16, 16, 8, 8)]
            d_counts = torch.zeros(2, dtype=torch.int32, device=dev)
            ws = CV.MCPEGenerator.MergeWorkspaceBytes(n)
            d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            times = []
            for _ in range(args.repeats + 1):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                gen.MergeDevice(d_records.data_ptr(), d_series.data_ptr(), d_series_counts.data_ptr(), n, window, outs[0].data_ptr(), outs[1].data_ptr(),
                                outs[2].data_ptr(), outs[3].data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws, stream=stream)
                stop.record()
                torch.cuda.synchronize()
                times.append(start.elapsed_time(stop) * 1e-3)
            assert [int(c) for c in d_counts.cpu()] == [len(want[0]), len(want[2])]
            assert outs[0].cpu().numpy()[:len(want[0]) * 16].tobytes() == want[0].tobytes() and outs[2].cpu().numpy()[:len(want[2]) * 8].tobytes() == want[2].tobytes()
            line.update(device_seconds=min(times[1:]), device_records_per_s=n / min(times[1:]))
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--series", type=int, default=0, metavar="N")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--pmt", action="store_true")
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--union", type=int, nargs=2, default=None, metavar=("N", "M"))
    ap.add_argument("--frame-photon-union", type=int, nargs=2, default=None, metavar=("N", "M"))
    ap.add_argument("--one-dom", action="store_true")
    ap.add_argument("--pmt-hit-union", type=int, nargs=2, default=None, metavar=("N", "M"))
    ap.add_argument("--one-channel", action="store_true")
    ap.add_argument("--pmt-series", type=int, default=0, metavar="N")
    ap.add_argument("--frame-photons", type=int, default=0, metavar="N")
    ap.add_argument("--cable-shadow", type=int, default=0, metavar="N")
    ap.add_argument("--cylinders", type=int, default=5160)
    ap.add_argument("--event-statistics", type=int, default=0, metavar="N")
    ap.add_argument("--photon-hits", type=int, default=0, metavar="N")
    ap.add_argument("--pmt-photon-hits", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if args.union:
        return union_rate(args)
    if args.frame_photon_union:
        return frame_photon_union_rate(args)
    if args.pmt_hit_union:
        return pmt_hit_union_rate(args)
    if args.pmt_photon_hits:
        return pmt_photon_hits_rate(args)
    if args.photon_hits:
        return photon_hits_rate(args)
    if args.event_statistics:
        return event_statistics_rate(args)
    if args.cable_shadow:
        return cable_shadow_rate(args)
    if args.frame_photons:
        return frame_photons_rate(args)
    if args.pmt_series:
        return pmt_series_rate(args)
    if args.merge:
        return merge_rate(args)
    if args.series:
        return series_rate(args)
    base = np.concatenate([M.fixture_photons(name) for name in M.FIXTURES if name != "lea_no_pancake"])     # recorded with pancake 5
    ph = np.ascontiguousarray(np.tile(base, -(-args.records // len(base)))[:args.records])
    if args.pmt:
        from tests import pmt_common as PC
        gen = PC.make_generator(*PC.configuration("identity", PC.sphere_radius_of("mie")))
        best = float("inf")
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            hits, counters = gen.ConvertHost(ph)
            best = min(best, time.perf_counter() - t0)
            assert not any(counters.values())
        print(json.dumps({"records": len(ph), "pmt_hits": len(hits), "pmts_per_module": 31, "seconds": best, "records_per_s": len(ph) / best, "threads": 1}))
        return
    gen = M.standard_generator()
    out = np.zeros(len(ph), dtype=CV.MCPE_DTYPE)
    n, counters = C.c_size_t(), np.zeros(4, dtype=np.uint64)
    lib = _lib.load()
    best = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        rc = lib.clsimhip_mcpe_convert_host(gen._h, ph.ctypes.data_as(C.c_void_p), len(ph), out.ctypes.data_as(C.c_void_p), len(out),
                                            C.byref(n), counters.ctypes.data_as(C.c_void_p))
        best = min(best, time.perf_counter() - t0)
        assert rc == 0 and not counters.any()
    print(json.dumps({"records": len(ph), "mcpes": n.value, "seconds": best, "records_per_s": len(ph) / best, "threads": 1}))


if __name__ == "__main__":
    main()
