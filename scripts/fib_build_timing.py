"""What a publish costs with the DIR-24-8 tables built on the device
(DP_OPT_DEVICE_FIB = 1, leg "on"), with the routes also sorted and listed there
(= 2, leg "sort"), and with the host building and uploading everything ("off").

The tables are C2's at BASELINE sizes (1M v4 routes), as bench.py publishes
them.  After one warm-up publish per leg the legs alternate, --runs
publishes each through GpuPathNf.publish on one context; per publish the host
clock around the call and the record of dp_tables_publish_stats (phase times,
bytes uploaded, bytes and event time of the build kernels).  Per leg: medians,
minimum and maximum of the wall time, medians of the phases.  A dp_fib_lookup
over random keys after the last publish of each leg must give the same answers
(the two images hold the same tables).

Prints one JSON line (and writes it to --out).  Nothing here is a pass / fail
threshold.  The kernels' split comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/fib_build_timing.py --runs 2`:
dp_fibbuild_direct_k, dp_fibbuild_blocks_k, and the dp_fibsort_*_k of mode 2."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("sort_us", "paint_us", "compile_us", "upload_us", "kernel_ns", "total_us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--routes", type=int, default=0, help="v4 routes (0: the BASELINE size)")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    from dataplane_amd import GpuPathNf, _abi as A
    from dataplane_amd.workload import Workload

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script only measures on the device")
    torch.cuda.init()
    w = Workload(2, 1024, seed=1, layout="dpdk", **({"n_routes_v4": args.routes} if args.routes else {}))
    nf = GpuPathNf(0)
    rng = np.random.default_rng(1)
    keys = np.zeros(200_000, dtype=A.FIB_KEY)
    t = w.tables.contents
    keys["vrf_id"], keys["family"] = t.fibs[t.routes[0].fib].vrf_id, 4  # the FIB that holds the v4 routes
    keys["addr"][:, :4] = rng.integers(0, 256, (len(keys), 4))
    modes = {"off": 0, "on": 1, "sort": 2}  # DP_OPT_DEVICE_FIB
    legs = {leg: [] for leg in modes}
    answers = {}

    def publish(leg):
        nf.set_device_fib(modes[leg])
        t0 = time.perf_counter()
        nf.publish(w.tables)
        wall = 1e3 * (time.perf_counter() - t0)
        return wall, nf.publish_stats()

    for leg in legs:
        publish(leg)  # warm-up: code objects, the build stream, allocator pools
    for _ in range(args.runs):
        for leg in legs:
            legs[leg].append(publish(leg))
            answers[leg] = nf.fib_lookup(keys)
    if not (np.array_equal(answers["on"], answers["off"]) and np.array_equal(answers["sort"], answers["off"])):
        raise SystemExit("the device-built tables answer differently")
    res = {"routes_v4": int(args.routes or 1_000_000), "runs": args.runs, "tile": A.FIB_BUILD_TILE, "stage": A.FIB_BUILD_STAGE}
    for leg, runs in legs.items():
        wall, st = [r[0] for r in runs], runs[-1][1]
        res[leg] = {"wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
                    "wall_ms": wall, "device_fibs": int(st["device_fibs"]), "sorted_fibs": int(st["sorted_fibs"]), "image_bytes": int(st["image_bytes"]),
                    "upload_bytes": int(st["upload_bytes"]), "built_bytes": int(st["built_bytes"])}
        for p in PHASES:
            res[leg][p + "_median"] = statistics.median(int(r[1][p]) for r in runs)
    nf.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
