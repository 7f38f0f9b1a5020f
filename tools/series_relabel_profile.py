#!/usr/bin/env python3
"""The series relabel stage beside its yardstick: clsimhip_mcpe_series_relabel_device and clsimhip_mcpe_series_union_device with an
empty B on the same series form in HBM -- the union reads and writes every record once, as the relabel pass does -- at the same
record count, alternating in one process, HIP events around each call, after warm-up calls of both.  Prints one JSON line per size:
both rates in records per second (median and the spread over the repeats), their ratio, and the host twin's rate.  The events lie
behind a second of queued fills, so that the host's part of a call -- the map's check and copy, the launches -- is over before
the device gets to it and the events see the kernels alone; the host's part is timed by itself, with a clock around the call.

    python tools/series_relabel_profile.py [--records 1000000 10000000] [--map 100000] [--repeats 15] [--ties 64] [--frame-photons]

The input: synthetic MCPEs (tests/mcpe_series_common.py) over 84 DOMs and five frames, a share of them at whole nanoseconds, under
`--map` slice identifiers that the map sends to a tenth as many muons.  --ties K: every K-th record at a whole nanosecond, which
makes disturbed runs (their number is on the line) and so runs the kernels behind the copy; --ties 0: binary64 times as in real
data, no run is disturbed and those kernels return at once.  --frame-photons: the 48-byte records and their union instead.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clsim_amd import converter as CV           # noqa: E402
from tests import mcpe_series_common as S       # noqa: E402
from tests import series_relabel_common as R    # noqa: E402


def make_form(kind, n, n_map, ties, seed=11):
    """a series form of n records under identifiers [n_map / 10, n_map / 10 + n_map): the slices; the map sends them to [0, n_map / 10)"""
    rng = np.random.default_rng(seed)
    muons = max(n_map // 10, 1)
    r = np.zeros(n, dtype=R.DTYPE[kind])
    dom = rng.integers(0, len(S.DOM_STRINGS), n)
    r["stringID"], r["omID"] = S.DOM_STRINGS[dom], S.DOM_OMS[dom]
    r["id"] = muons + rng.integers(0, max(n_map, 1), n)
    r["time"] = rng.uniform(500.0, 4000.0, n)
    if ties:
        r["time"][: n // ties] = np.round(r["time"][: n // ties])
    if kind == "photon":
        for name in ("weight", "wavelength", "groupVelocity", "x", "y", "z", "theta", "phi"):
            r[name] = rng.random(n, dtype=np.float32)
    frames = np.asarray((50, 10, 40, 20, 30), dtype=np.uint32)[r["id"] % 5]
    records, series = R.form_of(kind, r, frames)
    m = R.relabel_map([(muons + k, k % muons) for k in range(n_map)])
    return records, series, m


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--ties", type=int, default=64)
    ap.add_argument("--frame-photons", action="store_true")
    args = ap.parse_args()
    kind = "photon" if args.frame_photons else "mcpe"
    size = R.DTYPE[kind].itemsize
    dev = torch.device("cuda", 0)
    union = CV.FramePhotonStore if args.frame_photons else CV.MCPEGenerator
    for n in args.records:
        records, series, m = make_form(kind, n, args.map, args.ties)
        relabeler = CV.SeriesRelabeler(m)
        new = records.copy()
        new["id"], _ = R.new_ids(new["id"], m)
        disturbed, runs = R.disturbed_runs(kind, new, series)
        t0 = time.perf_counter()
        twin = (relabeler.mcpe_series_host if kind == "mcpe" else relabeler.frame_photons_host)(records, series)
        host_seconds = time.perf_counter() - t0
        up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)
        d_records, d_series = up(records), up(np.concatenate([series, np.zeros(n - len(series), dtype=series.dtype)]))
        d_counts = torch.tensor([n, len(series), 0, 0, 0], dtype=torch.int32, device=dev)
        d_empty, d_empty_counts = torch.zeros(64, dtype=torch.uint8, device=dev), torch.zeros(5, dtype=torch.int32, device=dev)
        d_out, d_table, d_out_counts = torch.zeros(n * size, dtype=torch.uint8, device=dev), torch.zeros(n * 16, dtype=torch.uint8, device=dev), torch.zeros(5, dtype=torch.int32, device=dev)
        ws_relabel, ws_union = relabeler.workspace_bytes(n, size), union.UnionWorkspaceBytes(n, 1)
        d_ws = torch.zeros(max(ws_relabel, ws_union), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        call_relabel = relabeler.mcpe_series_device if kind == "mcpe" else relabeler.frame_photons_device

        def relabel():
            call_relabel(d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), n, d_out.data_ptr(), d_table.data_ptr(), d_out_counts.data_ptr(),
                         d_ws.data_ptr(), ws_relabel, stream=stream)

        def yardstick():
            union.UnionDevice(d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), n, d_empty.data_ptr(), d_empty.data_ptr(), d_empty_counts.data_ptr(), 1,
                              d_out.data_ptr(), d_table.data_ptr(), d_out_counts.data_ptr(), n, d_ws.data_ptr(), ws_union, stream=stream)

        d_fill = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
        host = {relabel: [], yardstick: []}

        def timed(call):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(8):                      # the device is busy while the host queues the call
                d_fill.zero_()
            start.record()
            t0 = time.perf_counter()
            call()
            host[call].append(time.perf_counter() - t0)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) * 1e-3

        for _ in range(3):
            timed(relabel), timed(yardstick)
        relabel()
        torch.cuda.synchronize()
        counts = d_out_counts.cpu().numpy().view(np.uint32).tolist()
        same = d_out.cpu().numpy()[:n * size].tobytes() == twin[0].tobytes()
        times = {"relabel": [], "union": []}
        for _ in range(args.repeats):               # alternating: what disturbs one disturbs the other
            times["relabel"].append(timed(relabel))
            times["union"].append(timed(yardstick))
        rate = {k: n / float(np.median(v)) for k, v in times.items()}
        print(json.dumps({"records": n, "record_bytes": size, "map": len(m), "series": len(series), "runs": runs, "disturbed_runs": len(disturbed),
                          "counts": counts, "equal_to_host_twin": same,
                          "relabel_records_per_second": rate["relabel"], "union_records_per_second": rate["union"], "ratio_relabel_to_union": rate["relabel"] / rate["union"],
                          "relabel_seconds_min_median_max": [min(times["relabel"]), float(np.median(times["relabel"])), max(times["relabel"])],
                          "union_seconds_min_median_max": [min(times["union"]), float(np.median(times["union"])), max(times["union"])],
                          "relabel_host_seconds_per_call": float(np.median(host[relabel])), "union_host_seconds_per_call": float(np.median(host[yardstick])),
                          "host_twin_records_per_second": n / host_seconds}), flush=True)


if __name__ == "__main__":
    main()
