"""What the per-VPC statistics stage (DP_OPT_VPC_STATS) costs a resident burst.

The C2 burst bench.py times (2M packets, DPDK layout, BASELINE table sizes),
device resident, with a meta array: (a) the option off -- the path as it was
before the stage existed -- and (b) the option on, alternating, HIP events on
the launch stream around each call, the median of --runs calls after a
warm-up.  Prints one JSON line (and writes it to --out).

The accumulate kernel's own time comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/vpc_stats_timing.py --on-only`
(scripts/kstats.py prints the CSV): kernel dp_vpc_stats_k beside the pipeline
kernel of the same launches.  The JSON carries the yardsticks to hold it
against: the 24 B a packet the kernel reads at the HBM peak, and one
same-address atomic per packet at 12 ns."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_GBPS = 8000.0      # MI355X peak (DESIGN.md §3 Roofline)
ATOMIC_NS = 12.0       # one same-address global atomic
READ_B = 24            # dp_pkt_out_t + the first 8 B of dp_pkt_meta_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--on-only", action="store_true", help="only option-on calls (the profiled run)")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    from dataplane_amd import GpuPathNf, _abi as A
    from dataplane_amd.workload import Workload

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script only measures on the device")
    dev = torch.device("cuda", 0)
    w = Workload(2, args.packets, seed=1, layout="dpdk")
    nf = GpuPathNf(0)
    nf.publish(w.tables)
    n = w.n
    pristine = torch.from_numpy(w.fresh_buf()).to(dev)
    b = torch.empty_like(pristine)
    dinp = torch.from_numpy(w.inp.view(np.uint8)).to(dev)
    dout = torch.zeros(n * A.PKT_OUT.itemsize, dtype=torch.uint8, device=dev)
    dmeta = torch.zeros(n * A.PKT_META.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream

    def call(on):
        nf.set_vpc_stats(on)
        with torch.cuda.stream(stream):
            b.copy_(pristine)  # the path rewrites the frames in place
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            nf.process_device(b.data_ptr(), b.numel(), dinp.data_ptr(), dout.data_ptr(), n, None, sptr,
                              dev_meta=dmeta.data_ptr())
            e1.record(stream)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    modes = [True] if args.on_only else [False, True]
    for _ in range(args.warmup):
        for on in modes:
            call(on)
    ms = {on: [] for on in modes}
    for _ in range(args.runs):
        for on in modes:  # alternating: both see the same neighbours
            ms[on].append(call(on))
    cells, lost = nf.vpc_stats(reset=True)
    nf.close()
    res = {"config": 2, "packets": n, "runs": args.runs,
           "on_ms_median": statistics.median(ms[True]), "on_ms_min": min(ms[True]),
           "cells": int(len(cells)), "lost": lost,
           "accounted_packets": int(cells["fwd_packets"].sum() + cells["drop_packets"].sum()),
           "yardstick_read_bytes": READ_B * n, "yardstick_hbm_us": READ_B * n / HBM_GBPS / 1e3,
           "yardstick_atomic_per_packet_us": ATOMIC_NS * n / 1e3}
    if False in ms:
        res.update(off_ms_median=statistics.median(ms[False]), off_ms_min=min(ms[False]),
                   delta_us_median=1e3 * (res["on_ms_median"] - statistics.median(ms[False])))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
