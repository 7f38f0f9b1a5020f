#!/usr/bin/env python3
"""One full C2 bunch (SPICE-Mie, IC86, 1 048 576 cascade steps of 200 photons) through the converter with the MCPE generator and
the MCPE series stage, steps dealt to 1000 particles in 10 frames: the run to put under `rocprofv3 --kernel-trace --stats` to see
the stage's kernels beside the propagation kernel.  Prints the counts and the host-side wall time of the bunch.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/mcpe_series_profile.py [--steps 1048576] [--no-series] [--merge-window NS]
                                                                                   [--pmt] [--frame-photons] [--cable-shadow]
                                                                                   [--event-statistics] [--photon-hits]
                                                                                   [--pmt-photon-hits] [--frame-store]
                                                                                   [--frame-photon-store]

--frame-store: a device MCPE frame store of 2^20 records folded behind each bunch (clsimhip_mcpe_frame_store_add_host: the upload
and the union kernels), drained at the end; the line then carries the store's sizes.
--frame-photon-store: with --frame-photons: a device frame photon store of 2^20 records folded behind each bunch
(clsimhip_frame_photon_store_add_host: the upload and the union kernels), drained up to frame 4 at the end; a second line carries the
store's sizes.
--merge-window NS: the MCPE merging stage behind the series stage, with that window.
--pmt: a 31-PMT module (tests/pmt_common.py) at every DOM instead: the multi-PMT hit maker and the PMT series stage (--no-series:
the hit maker alone).
--frame-photons: no hit maker; the frame photons stage on the bunch's photon records, which stay on the device (--no-series: the
propagation alone, records downloaded).
--photon-hits: with --frame-photons: the photon hits stage (IceCube acceptance, hole-ice angular acceptance, efficiencies from {0.5, 1,
1.35}, pancake 2 of oversize 5 so that the time correction is live) on the second bunch's frame photons, uploaded again and run
twice on the device (the first call copies the maker's tables); the line then carries the stage's counts.
--pmt-photon-hits: with --frame-photons: the PMT photon hits stage with a 31-PMT module (tests/pmt_common.py) at every DOM on the
second bunch's frame photons, in the same way; the process then runs --pmt's two bunches as well (the online hit maker and the PMT
series stage, a second line), so that one trace holds pmt_hits_kernel and the PMT series' kernels beside this stage's.
--cable-shadow: the cable shadow stage in front of whichever stages the other options choose, with one cable beside every DOM of
the geometry (5 160 cylinders, in the DOM's own frame: tests/cable_shadow_common.py); the line then carries its two counts.
--event-statistics: the event statistics stage beside whichever stages the other options choose (with --no-series the bunch has no
particle table and yields one record); the line then carries the records, the photons at DOMs and the stage's counters.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clsim_amd import converter as CV           # noqa: E402
from tests import common                        # noqa: E402
from tests import mcpe_common as M              # noqa: E402


def cable_shadow_of(args, cfg):
    if not args.cable_shadow:
        return None
    from tests import cable_shadow_common as S
    return S.make_shadow(S.cylinder_set(len(cfg["geom"]["string_ids"])))


def event_statistics_of(r):
    if not hasattr(r, "event_statistics"):
        return None
    return {"records": len(r.event_statistics), "at_doms": int(r.event_statistics["atDOMsCount"].sum()),
            "generated": int(r.event_statistics["generatedCount"].sum()), "counters": r.event_statistics_counters}


def pmt_bunch(args, cfg, bias):
    from tests import pmt_common as PC
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias), pancakeFactor=5.0,
                            stopDetectedPhotons=True, approximateNumberOfWorkItems=args.steps, pmtHitGenerator=PC.geometry_generator(cfg),
                            keepPhotons=False, pmtSeries=not args.no_series, cableShadow=cable_shadow_of(args, cfg), eventStatistics=args.event_statistics)
    steps = common.steps_for(cfg, args.steps, seed=3).copy()
    steps["id"] = np.arange(len(steps)) % 1000
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, np.arange(1000) * 1000.0
    for bunch in range(2):          # the first bunch allocates the pools
        t0 = time.perf_counter()
        if args.no_series:
            conv.EnqueueSteps(steps, bunch)
        else:
            conv.EnqueueSteps(steps, bunch, particles=p)
        r = conv.GetConversionResult()
        wall = time.perf_counter() - t0
    print(json.dumps({"steps": len(steps), "photons": int(steps["num"].sum()), "pmt_hits": len(r.pmt_hits),
                      "pmt_series": None if r.pmt_series is None else len(r.pmt_series), "cable_shadow": r.shadow_counts, "event_statistics": event_statistics_of(r), "wall_seconds_second_bunch": wall}))


def photon_hits_of(cfg, r):
    """the photon hits stage on the result's frame photons, on the device; {kept, series, counters}"""
    import torch
    from tests import photon_hits_common as P
    g = cfg["geom"]
    maker = P.maker_of(P.spec(P.dom_table(np.asarray(g["string_ids"]), np.asarray(g["dom_ids"]), efficiencies=(0.5, 1.0, 1.35), spe=1.0), pancake=2.0))
    dev = torch.device("cuda", 0)
    n = len(r.frame_photons)
    d_records = torch.from_numpy(r.frame_photons.view(np.uint8).copy()).to(dev)
    d_series = torch.from_numpy(r.frame_photon_series.view(np.uint8).copy()).to(dev)
    d_in = torch.tensor([n, len(r.frame_photon_series)], dtype=torch.int32, device=dev)
    d_out, d_out_series = torch.empty(max(n, 1) * 16, dtype=torch.uint8, device=dev), torch.empty(max(n, 1) * 16, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(9, dtype=torch.int32, device=dev)
    ws_bytes = CV.PhotonHitMaker.WorkspaceBytes(n)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    for _ in range(2):
        maker.MakeHitsDevice(d_records.data_ptr(), d_series.data_ptr(), d_in.data_ptr(), n, d_out.data_ptr(), d_out_series.data_ptr(), d_counts.data_ptr(),
                             d_ws.data_ptr(), ws_bytes, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    counts = [int(c) for c in d_counts.cpu().numpy()]
    return {"records": n, "kept": counts[0], "series": counts[1], "counters": dict(zip(CV.PHOTON_HIT_COUNTERS, counts[2:]))}


def pmt_photon_hits_of(cfg, r):
    """the PMT photon hits stage on the result's frame photons, on the device; {kept, series, counters}"""
    import torch
    from tests import pmt_common as PC
    gen = PC.geometry_generator(cfg)
    dev = torch.device("cuda", 0)
    n = len(r.frame_photons)
    d_records = torch.from_numpy(r.frame_photons.view(np.uint8).copy()).to(dev)
    d_series = torch.from_numpy(r.frame_photon_series.view(np.uint8).copy()).to(dev)
    d_in = torch.tensor([n, len(r.frame_photon_series)], dtype=torch.int32, device=dev)
    d_out, d_out_series = torch.empty(max(n, 1) * 24, dtype=torch.uint8, device=dev), torch.empty(max(n, 1) * 24, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(7, dtype=torch.int32, device=dev)
    ws_bytes = CV.PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(n)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    for _ in range(2):
        gen.MakeHitsFromFramePhotonsDevice(d_records.data_ptr(), d_series.data_ptr(), d_in.data_ptr(), n, d_out.data_ptr(), d_out_series.data_ptr(),
                                           d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    counts = [int(c) for c in d_counts.cpu().numpy()]
    return {"records": n, "kept": counts[0], "series": counts[1], "counters": dict(zip(CV.PMT_PHOTON_HIT_COUNTERS, counts[2:]))}


def frame_photons_bunch(args, cfg, bias):
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(cfg["geom"]), cfg["med_p"], bias, common.product_generators(cfg, bias), pancakeFactor=5.0,
                            stopDetectedPhotons=True, approximateNumberOfWorkItems=args.steps, keepPhotons=False, framePhotons=not args.no_series,
                            cableShadow=cable_shadow_of(args, cfg), eventStatistics=args.event_statistics)
    steps = common.steps_for(cfg, args.steps, seed=3).copy()
    steps["id"] = np.arange(len(steps)) % 1000
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, np.arange(1000) * 1000.0
    store = CV.FramePhotonStore(1 << 20, device=0) if args.frame_photon_store and not args.no_series else None
    for bunch in range(2):          # the first bunch allocates the pools
        t0 = time.perf_counter()
        if args.no_series:
            conv.EnqueueSteps(steps, bunch)
        else:
            conv.EnqueueSteps(steps, bunch, particles=p)
        r = conv.GetConversionResult()
        if store is not None:
            store.Add(r.frame_photons, r.frame_photon_series)
        wall = time.perf_counter() - t0
    if store is not None:
        stored = store.Size()
        head = store.Drain(4)
        print(json.dumps({"frame_photon_store_records": stored[0], "frame_photon_store_series": stored[1], "drained_up_to_frame_4": len(head[0]), "left": store.Size()[0]}))
    hits = photon_hits_of(cfg, r) if args.photon_hits and r.frame_photons is not None else None
    pmt_hits = pmt_photon_hits_of(cfg, r) if args.pmt_photon_hits and r.frame_photons is not None else None
    print(json.dumps({"steps": len(steps), "photons": int(steps["num"].sum()), "photon_records": len(r[1]), "photon_hits": hits, "pmt_photon_hits": pmt_hits,
                      "frame_photons": None if r.frame_photons is None else len(r.frame_photons),
                      "frame_photon_series": None if r.frame_photon_series is None else len(r.frame_photon_series), "cable_shadow": r.shadow_counts,
                      "event_statistics": event_statistics_of(r), "wall_seconds_second_bunch": wall}))
    if pmt_hits is not None:
        del conv, r
        pmt_bunch(args, cfg, bias)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1 << 20)
    ap.add_argument("--no-series", action="store_true")
    ap.add_argument("--merge-window", type=float, default=None, metavar="NS")
    ap.add_argument("--pmt", action="store_true")
    ap.add_argument("--frame-photons", action="store_true")
    ap.add_argument("--cable-shadow", action="store_true")
    ap.add_argument("--event-statistics", action="store_true")
    ap.add_argument("--photon-hits", action="store_true")
    ap.add_argument("--pmt-photon-hits", action="store_true")
    ap.add_argument("--frame-store", action="store_true")
    ap.add_argument("--frame-photon-store", action="store_true")
    args = ap.parse_args()
    if args.frame_photon_store and (not args.frame_photons or args.no_series or args.pmt):
        ap.error("--frame-photon-store needs --frame-photons with the stage on (no --no-series, no --pmt): there would be nothing to store")
    cfg = common.config("mie")
    g = cfg["geom"]
    s, d = np.asarray(g["string_ids"]), np.asarray(g["dom_ids"])
    gen = M.make_generator([M.acceptance_table()], s, d, np.zeros(len(s), dtype=np.int32))
    bias = CV.GetIceCubeDOMAcceptance()
    if args.pmt:
        return pmt_bunch(args, cfg, bias)
    if args.frame_photons:
        return frame_photons_bunch(args, cfg, bias)
    conv = CV.initializeHIP(0, CV.I3CLSimSimpleGeometry.from_dict(g), cfg["med_p"], bias, common.product_generators(cfg, bias), pancakeFactor=5.0,
                            stopDetectedPhotons=True, approximateNumberOfWorkItems=args.steps, mcpeGenerator=gen, keepPhotons=False,
                            mcpeSeries=not args.no_series, mcpeMergeWindow=args.merge_window, cableShadow=cable_shadow_of(args, cfg), eventStatistics=args.event_statistics)
    steps = common.steps_for(cfg, args.steps, seed=3).copy()
    steps["id"] = np.arange(len(steps)) % 1000
    p = np.zeros(1000, dtype=CV.MCPE_PARTICLE_DTYPE)
    p["id"], p["frame"], p["timeShift"] = np.arange(1000), np.arange(1000) % 10, np.arange(1000) * 1000.0
    store = CV.MCPEFrameStore(1 << 20, device=0) if args.frame_store and not args.no_series else None
    for bunch in range(2):          # the first bunch allocates the pools
        t0 = time.perf_counter()
        if args.no_series:
            conv.EnqueueSteps(steps, bunch)
        else:
            conv.EnqueueSteps(steps, bunch, particles=p)
        r = conv.GetConversionResult()
        if store is not None:
            store.Add(r.mcpes, r.series)
        wall = time.perf_counter() - t0
    if store is not None:
        stored = store.Size()
        head = store.Drain(4)
        print(json.dumps({"frame_store_records": stored[0], "frame_store_series": stored[1], "drained_up_to_frame_4": len(head[0]), "left": store.Size()[0]}))
    print(json.dumps({"steps": len(steps), "photons": int(steps["num"].sum()), "mcpes": len(r.mcpes),
                      "series": None if r.series is None else len(r.series),
                      "merged": None if r.merged is None else len(r.merged), "parents": None if r.parents is None else len(r.parents),
                      "cable_shadow": r.shadow_counts, "event_statistics": event_statistics_of(r), "wall_seconds_second_bunch": wall}))


if __name__ == "__main__":
    main()
