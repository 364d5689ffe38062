"""What dp_flow_snapshot takes on a large table, beside dp_flow_count.

One process, one table of --slots slots (2^24: 2 GiB), filled in two steps
(--fills, 5 % then 40 %) with distinct v4 UDP flows.  At each fill the calls
below run alternating, round-robin, --runs rounds after --warmup, and the
median and the spread (min, max) of each are reported:

  count            dp_flow_count: the yardstick (one lane per slot, one dword per line)
  count_first      count-only snapshot, first-half clauses (family, src prefix)
  count_second     count-only snapshot, a second-half clause (genid <)
  snap_1pct        the 1 % of the flows with a marked dst_vni, into device memory
  snap_all_device  every flow into device memory
  snap_all_host    every flow into host memory (the copy included; --host-runs)

The calls are synchronous and launch on the table's own stream, so the clock
is the host's around each call (launches and the final synchronisation
included, for the yardstick as well).  `bytes` is what the scan must move:
64 B per slot scanned, 64 B more per slot that passes the first-half clauses
when the filter has a second-half clause or the slot is emitted, 136 B per
entry written; `hbm_frac` is bytes / time over --hbm-gbs.  dp_flow_count's
useful bytes are 8 per slot (two dwords); it moves a line per slot all the
same.  Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flows_range(A, lo, hi):
    """Flows number lo..hi-1: distinct sources 10.x.y.z / 11.x.y.z, 1 % with dst_vni 100."""
    i = np.arange(lo, hi, dtype=np.uint32)
    fl = np.zeros(len(i), A.FLOW)
    k = fl["key"]
    k["src_vni"], k["family"], k["kind"] = 1 + i % 1000, 4, A.FLOW_UDP
    k["sport"], k["dport"] = 1 + i % 60000, 53
    k["src"][:, 0] = 10 + (i >> 24)
    for b in range(3):
        k["src"][:, 1 + b] = (i >> (16 - 8 * b)) & 255
    k["dst"][:, :4] = (192, 0, 2, 1)
    fl["dst_vni"] = np.where(i % 100 == 0, 100, 5)
    fl["genid"], fl["expires_at"] = i % 8, (1 << 63) - 1
    return fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1 << 24)
    ap.add_argument("--fills", default="0.05,0.40")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default="profiles/flow_snapshot/timing.json")
    args = ap.parse_args()

    import torch
    from dataplane_amd import _abi as A
    from dataplane_amd.flows import FlowTable, flow_filter

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script only measures on the device")
    torch.cuda.init()
    ft = FlowTable(0, args.slots)
    first = flow_filter(family=4, src="10.0.0.0/9")
    second = flow_filter(genid_lt=4)
    marked = flow_filter(dst_vni=100)
    doc = dict(slots=args.slots, hbm_gbs=args.hbm_gbs, runs=args.runs, fills=[])
    have = 0
    for fill in (float(x) for x in args.fills.split(",")):
        n = int(args.slots * fill)
        for lo in range(have, n, 1 << 20):
            _, res = ft.insert(flows_range(A, lo, min(n, lo + (1 << 20))))
            assert (res == A.FLOW_INSERTED).all()
        have = n
        assert ft.count()[0] == n
        n_first, n_second, n_marked = (ft.count_matching(f) for f in (first, second, marked))
        dbuf = torch.empty(n * A.FLOW_ENTRY.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        S, E = 64 * args.slots, A.FLOW_ENTRY.itemsize
        calls = dict(
            count=(ft.count, 8 * args.slots),
            count_first=(lambda: ft.count_matching(first), S),
            count_second=(lambda: ft.count_matching(second), S + 64 * n),
            snap_1pct=(lambda: ft.snapshot_page(marked, 0, n, device_ptr=dbuf.data_ptr()), S + (64 + E) * n_marked),
            snap_all_device=(lambda: ft.snapshot_page(None, 0, n, device_ptr=dbuf.data_ptr()), S + (64 + E) * n),
            snap_all_host=(lambda: ft.snapshot_page(None, 0, n), S + (64 + E) * n))
        times = {name: [] for name in calls}
        for r in range(args.warmup + args.runs):
            for name, (call, _) in calls.items():
                if name == "snap_all_host" and r >= args.host_runs:
                    continue
                t0 = time.perf_counter()
                call()
                if r >= args.warmup or name == "snap_all_host":
                    times[name].append(time.perf_counter() - t0)
        rec = dict(fill=fill, flows=n, matches=dict(first=n_first, second=n_second, marked=n_marked), calls={})
        for name, (_, nbytes) in calls.items():
            med = statistics.median(times[name])
            rec["calls"][name] = dict(us=round(med * 1e6, 1), min_us=round(min(times[name]) * 1e6, 1),
                                      max_us=round(max(times[name]) * 1e6, 1), bytes=nbytes,
                                      gbs=round(nbytes / med / 1e9, 1),
                                      hbm_frac=round(nbytes / med / 1e9 / args.hbm_gbs, 3))
        doc["fills"].append(rec)
        print(json.dumps(rec), flush=True)
        del dbuf
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
