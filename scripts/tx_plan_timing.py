"""What the TX plan (dp_tx_plan_device) costs a resident burst, and what it replaces.

Two inputs of --packets dp_pkt_out_t records, device resident:

  c2        -- the records of the C2 burst bench.py times (DPDK layout, BASELINE
               table sizes), planned over the ports its Delivered packets name
               (at most DP_TX_MAX_PORTS);
  uniform32 -- synthetic records, all Delivered, spread evenly over 32 ports.

Per input: dp_tx_plan_device alone (its three kernels together), HIP events on
the launch stream around each call, the median and minimum of --runs calls
after a warm-up.  Beside them, from the same call of this script:

  pipeline  -- dp_process_burst_device over the C2 burst, timed the same way
               (--burst-runs calls);
  host      -- the alternative the plan replaces, two figures: the D2H copy of
               the records into pinned memory (host clock around the copy and
               its synchronise), and numpy's bucket ids + stable argsort over
               them (host clock; no per-port byte sums).

Prints one JSON line (and writes it to --out).  Nothing here is a pass / fail
threshold.  The split into the three kernels comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/tx_plan_timing.py --leg c2`
(or uniform32): dp_txplan_count_k, _scan_k, _scatter_k."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--burst-runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--leg", choices=["c2", "uniform32"], help="only that input's plan launches (the profiled run)")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    from dataplane_amd import GpuPathNf, _abi as A
    from dataplane_amd.workload import Workload

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script only measures on the device")
    dev = torch.device("cuda", 0)
    delivered = A.DONE["Delivered"]
    w = Workload(2, args.packets, seed=1, layout="dpdk")
    nf = GpuPathNf(0)
    nf.publish(w.tables)
    n = w.n
    pristine = torch.from_numpy(w.fresh_buf()).to(dev)
    b = torch.empty_like(pristine)
    dinp = torch.from_numpy(w.inp.view(np.uint8)).to(dev)
    dout = torch.zeros(n * A.PKT_OUT.itemsize, dtype=torch.uint8, device=dev)
    dorder = torch.zeros(n, dtype=torch.int32, device=dev)
    dports = torch.zeros((A.TX_MAX_PORTS + 2) * A.TX_PORT.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream

    def timed(fn):
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def burst():
        with torch.cuda.stream(stream):
            b.copy_(pristine)  # the path rewrites the frames in place
        return timed(lambda: nf.process_device(b.data_ptr(), b.numel(), dinp.data_ptr(), dout.data_ptr(), n, None,
                                               sptr))

    def buckets(out, oifs):
        """The contract's bucket id per record, as a host would compute it."""
        ok = out["done"] == delivered
        bucket = np.where(ok, len(oifs), len(oifs) + 1).astype(np.uint8)
        order = np.argsort(oifs)
        pos = np.minimum(np.searchsorted(oifs[order], out["oif"]), max(len(oifs) - 1, 0))
        hit = ok & (len(oifs) > 0) & (oifs[order][pos] == out["oif"]) if len(oifs) else np.zeros(len(out), bool)
        bucket[hit] = order[pos[hit]]
        return bucket

    res = {"packets": n, "runs": args.runs, "tile": A.TX_PLAN_TILE}
    ms = [burst() for _ in range(args.warmup + args.burst_runs)][args.warmup:]
    res.update(pipeline_c2_ms_median=statistics.median(ms), pipeline_c2_ms_min=min(ms), pipeline_runs=args.burst_runs)
    c2 = dout.cpu().numpy().view(A.PKT_OUT).copy()
    c2_oifs = np.unique(c2["oif"][(c2["done"] == delivered) & (c2["oif"] != 0)])[:A.TX_MAX_PORTS].astype(np.uint32)
    rng = np.random.default_rng(1)
    uni = np.zeros(n, dtype=A.PKT_OUT)
    uni["len"], uni["done"] = rng.integers(64, 1515, n), delivered
    uni_oifs = (1 + rng.permutation(32)).astype(np.uint32)
    uni["oif"] = uni_oifs[rng.integers(0, 32, n)]
    duni = torch.from_numpy(uni.view(np.uint8)).to(dev)
    hpin = torch.empty(n * A.PKT_OUT.itemsize, dtype=torch.uint8).pin_memory()

    for name, recs, drecs, oifs in (("c2", c2, dout, c2_oifs), ("uniform32", uni, duni, uni_oifs)):
        if args.leg and args.leg != name:
            continue
        plan = lambda: nf.tx_plan_device(drecs.data_ptr(), n, oifs, dorder.data_ptr(), dports.data_ptr(), sptr)
        us = [1e3 * timed(plan) for _ in range(args.warmup + args.runs)][args.warmup:]
        res["plan_%s_us_median" % name], res["plan_%s_us_min" % name] = statistics.median(us), min(us)
        res["plan_%s_ports" % name] = len(oifs)
        ports = dports.cpu().numpy().view(A.TX_PORT)[:len(oifs) + 2]
        res["plan_%s_counts_min_max_drop_free" % name] = [
            int(ports["count"][:len(oifs)].min()) if len(oifs) else 0,
            int(ports["count"][:len(oifs)].max()) if len(oifs) else 0,
            int(ports["count"][-2]), int(ports["count"][-1])]
        if args.leg:
            continue
        # the plan must be the one the host alternative computes
        ref = np.argsort(buckets(recs, oifs), kind="stable")
        if not np.array_equal(dorder.cpu().numpy().view(np.uint32), ref):
            raise SystemExit("plan of %s differs from the host's" % name)
        d2h, sort = [], []
        for _ in range(args.host_runs):
            t0 = time.perf_counter()
            hpin.copy_(drecs, non_blocking=True)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            np.argsort(buckets(hpin.numpy().view(A.PKT_OUT), oifs), kind="stable")
            t2 = time.perf_counter()
            d2h.append(1e3 * (t1 - t0)), sort.append(1e3 * (t2 - t1))
        res["host_%s_d2h_records_ms_median" % name] = statistics.median(d2h)
        res["host_%s_numpy_bucket_argsort_ms_median" % name] = statistics.median(sort)
    nf.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
