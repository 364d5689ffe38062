"""What dp_fib_lookup_device takes per kernel form, on the images bench.py uses.

Per config (2: 1M v4 routes, DIR-24-8; 5: v6 under one /32, window table) the
workload's tables are published and --keys device-resident keys are looked up
in the FIB that holds the routes (the last FIB, the destination VPC's), over
three key streams: the workload's own packet destinations in burst order, the
same sorted by destination, and uniform random addresses.  Each stream runs
per kernel form (forced direct and auto; the binned form this script measured
against them was removed), alternating, HIP events on the launch
stream around each call, the median of --runs calls after a warm-up; the
forms' results are compared once.  Prints one JSON line per
config (and appends it to --out).

bytes_per_key: the 24 B key and 8 B result every lookup streams, plus (v4,
DIR-24-8 with 4-byte entries) the distinct 64-byte lines of the direct table
the stream touches, spread over its keys -- the table traffic of a perfect
cache.  The kernel's own time comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/fib_lookup_timing.py ...`
(scripts/kstats.py prints the CSV): kernel dp_fib_lookup_k."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = {"auto": 0, "direct": 1}


def destinations(w, fam):
    """(n, 4 | 16) destination address bytes of the workload's frames of that
    family, in burst order (plain Ethernet + IP: the overlay configs seed the
    source VPC, no VXLAN header); a mixed burst's frames of the family are
    repeated up to n."""
    buf, off = w.fresh_buf(), w.inp["off"].astype(np.int64)
    nb, at, et = (4, 14 + 16, 0x0800) if fam == 4 else (16, 14 + 24, 0x86DD)
    off = off[(buf[off + 12].astype(np.int64) << 8 | buf[off + 13]) == et]
    return np.resize(buf[off[:, None] + at + np.arange(nb)[None, :]], (len(w.inp), nb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--forms", default="direct,auto")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    from dataplane_amd import GpuPathNf, _abi as A
    from dataplane_amd.workload import Workload

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script only measures on the device")
    dev = torch.device("cuda", 0)
    lib = A.gpu_lib()
    forms = args.forms.split(",")
    for cfg in [int(c) for c in args.configs.split(",")]:
        fam = 6 if cfg == 5 else 4
        w = Workload(cfg, args.keys, seed=1, layout="dpdk")
        nf = GpuPathNf(0)
        nf.publish(w.tables)
        d = w.tables.contents
        vrf = int(d.fibs[d.n_fibs - 1].vrf_id)
        n = w.n
        dst = destinations(w, fam)
        order = np.lexsort(dst.T[::-1])
        rng = np.random.default_rng(1)
        streams = {"burst": dst, "sorted": dst[order],
                   "uniform": rng.integers(0, 256, dst.shape, dtype=np.uint8)}
        stream = torch.cuda.Stream(dev)
        dout = torch.zeros(n * A.FIB_RESULT.itemsize, dtype=torch.uint8, device=dev)
        res = {"config": cfg, "family": fam, "keys": n, "runs": args.runs, "vrf": vrf, "streams": {}}
        for sname, addr in streams.items():
            keys = np.zeros(n, dtype=A.FIB_KEY)
            keys["vrf_id"], keys["family"] = vrf, fam
            keys["addr"][:, :addr.shape[1]] = addr
            dk = torch.from_numpy(keys.view(np.uint8)).to(dev)

            def call(form):
                lib.dpd_debug_set_fib_lookup_form(FORMS[form])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                nf.fib_lookup_device(dk.data_ptr(), dout.data_ptr(), n, stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                return e0.elapsed_time(e1)

            got = {}
            for _ in range(args.warmup):
                for f in forms:
                    call(f)
                    got[f] = dout.clone()
            agree = all(torch.equal(got[forms[0]], g) for g in got.values())
            ms = {f: [] for f in forms}
            for _ in range(args.runs):
                for f in forms:  # alternating: every form sees the same neighbours
                    ms[f].append(call(f))
            codes = got[forms[0]].cpu().numpy().view(A.FIB_RESULT)["code"]
            bpk = 32.0
            if fam == 4:
                lines = np.unique(addr[:, :3].astype(np.uint32) @ np.array([65536, 256, 1], dtype=np.uint32) >> 4)
                bpk += 64.0 * len(lines) / n
            res["streams"][sname] = {
                "forms_agree": bool(agree), "routes_hit": int((codes == A.FIB_ROUTE).sum()),
                "bytes_per_key": round(bpk, 2),
                **{f: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                       "mlookups_s": round(n / statistics.median(v) / 1e3, 1)} for f, v in ms.items()}}
        lib.dpd_debug_set_fib_lookup_form(0)
        nf.close()
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
