"""Per step of a rocprofv3 kernel trace of bench.py (kernel_trace.csv): the
pipeline kernel's duration, dp_stats_reduce's where a launch has one, and the
idle gaps pipeline end -> reduce start and last kernel end -> next pipeline
start.  Medians over the last STEPS pipeline dispatches (the timed steps:
warm-up and restaging copies come before them), in us.

    python scripts/dev/launch_gaps.py kernel_trace.csv [STEPS]
"""
import csv
import json
import sys


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else None


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ev = []
    for r in rows:
        name = r["Kernel_Name"]
        kind = "pipe" if "dp_pipeline_kernel" in name else "reduce" if "dp_stats_reduce" in name else None
        if kind:
            ev.append((kind, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    pipes = [k for k, e in enumerate(ev) if e[0] == "pipe"][-steps:]
    ev = ev[pipes[0]:]
    pipe, red, gap_pr, gap_next, period = [], [], [], [], []
    last_end, last_pipe = None, None
    for kind, a, b in ev:
        if kind == "pipe":
            if last_end is not None:
                gap_next.append(a - last_end)
                period.append(a - last_pipe)
            pipe.append(b - a)
            last_pipe = a
        else:
            red.append(b - a)
            gap_pr.append(a - last_end)
        last_end = b
    us = lambda v: None if median(v) is None else round(median(v) / 1e3, 2)
    print(json.dumps({"steps": len(pipe), "reduce_launches": len(red), "pipeline_us": us(pipe),
                      "reduce_us": us(red), "gap_pipeline_to_reduce_us": us(gap_pr),
                      "gap_to_next_pipeline_us": us(gap_next), "pipeline_start_to_start_us": us(period),
                      "pipeline_us_mean": round(sum(pipe) / len(pipe) / 1e3, 2),
                      "start_to_start_us_mean": round(sum(period) / len(period) / 1e3, 2) if period else None}))


if __name__ == "__main__":
    main()
