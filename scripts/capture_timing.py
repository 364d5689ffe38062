"""What packet capture (DP_OPT_CAPTURE, dp_capture_device) costs a resident burst.

The C2 burst bench.py times (2M packets, DPDK layout, BASELINE table sizes),
device resident, with a meta array:

  burst   -- dp_process_burst_device with the option off and with the TX tap on
             (every packet, snaplen 128), alternating, HIP events on the launch
             stream around each call, the median of --runs calls after a warm-up;
  capture -- dp_capture_device alone (its three kernels together) over the
             burst's TX records for (a) a source-port range that selects about
             1 % of the packets, snaplen 0, and (b) every packet, snaplen 128,
             the buffer reset between calls;
  yardsticks of the same run -- the burst with the option off (the pipeline
             kernel and nothing else) and a device-to-device hipMemcpyAsync of
             as many bytes as (b) stores.

Prints one JSON line (and writes it to --out).  The split into the three
kernels comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/capture_timing.py --leg a`
(or b; scripts/kstats.py prints the CSV): dp_capture_select_k, _scan_k, _copy_k."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", choices=["a", "b"], help="only that filter's capture launches (the profiled run)")
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

    fa, fb = np.zeros((), dtype=A.CAP_FILTER), np.zeros((), dtype=A.CAP_FILTER)
    fa["clauses"], fa["sport_lo"], fa["sport_hi"] = A.CAPF_SPORT, 0, 6553  # (the JSON carries what it selected)
    fb["snaplen"] = 128
    nf.capture_open(fb, n, 128 * n)

    def timed(fn):
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def burst(taps):
        nf.set_capture(taps)
        with torch.cuda.stream(stream):
            b.copy_(pristine)  # the path rewrites the frames in place
        ms = timed(lambda: nf.process_device(b.data_ptr(), b.numel(), dinp.data_ptr(), dout.data_ptr(), n, None,
                                             sptr, dev_meta=dmeta.data_ptr()))
        nf.set_capture(0)
        return ms

    import ctypes as C
    hrecs, hbytes = np.zeros(n, dtype=A.CAP_REC), np.zeros(128 * n, dtype=np.uint8)

    def drain():
        """(records, bytes) the buffer held; emptied."""
        nr, nb = C.c_uint32(0), C.c_uint64(0)
        A.check(nf.lib.dp_capture_read(nf.ctx, hrecs.ctypes.data, n, hbytes.ctypes.data, hbytes.nbytes, C.byref(nr),
                                       C.byref(nb), None, None, 1), "dp_capture_read", nf.lib)
        return nr.value, nb.value

    def capture(f):
        nf.set_capture_filter(f)
        ms = timed(lambda: nf.capture_device(A.CAP_TX, b.data_ptr(), b.numel(), dout.data_ptr(), dmeta.data_ptr(),
                                             n, sptr))
        return (ms,) + drain()

    burst(0)  # the records the capture legs read
    res = {"config": 2, "packets": n, "runs": args.runs}
    legs = {"a": fa, "b": fb}
    if args.leg:
        for _ in range(args.warmup + args.runs):
            capture(legs[args.leg])
        nf.close()
        return
    for _ in range(args.warmup):
        burst(0), burst(A.CAP_TX)
        drain()
    off, on = [], []
    for _ in range(args.runs):  # alternating: both see the same neighbours
        off.append(burst(0))
        on.append(burst(A.CAP_TX))
        drain()
    res.update(burst_off_ms_median=statistics.median(off), burst_off_ms_min=min(off),
               burst_tx_tap_ms_median=statistics.median(on), burst_tx_tap_ms_min=min(on),
               tap_delta_us_median=1e3 * (statistics.median(on) - statistics.median(off)))
    burst(0)
    for name, f in legs.items():
        ms, nr, nb = zip(*[capture(f) for _ in range(args.warmup + args.runs)][args.warmup:])
        res["capture_%s_us_median" % name] = 1e3 * statistics.median(ms)
        res["capture_%s_us_min" % name] = 1e3 * min(ms)
        res["capture_%s_records" % name], res["capture_%s_bytes" % name] = nr[0], nb[0]
    # yardstick: a device-to-device copy of as many bytes as (b) stores
    nbytes = res["capture_b_bytes"]
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d2d = [timed(lambda: dst.copy_(src)) for _ in range(args.warmup + args.runs)][args.warmup:]
    res.update(yardstick_d2d_bytes=nbytes, yardstick_d2d_us_median=1e3 * statistics.median(d2d),
               yardstick_pipeline_ms_median=res["burst_off_ms_median"])
    nf.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
