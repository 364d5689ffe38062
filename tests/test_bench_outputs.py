"""`bench.py --dump-outputs DIR`, `--full` and the timed steps.

CPU: dump_outputs over the oracle's result of a small burst -- the files, their
types and what they hold.  GPU: one plain run of the benchmark at a small size
with more steps than staged bursts (so the steps run in chunks): the result
line holds the headline fields and none of the --full legs, --steps is the
number of steps the histogram counted, and the dumped arrays equal the
oracle's over the same seeded workload."""
import json
import os
import subprocess
import sys
from importlib import util

import numpy as np
import pytest

from dataplane_amd import _abi as A
from dataplane_amd.shard import shard_seed
from dataplane_amd.workload import Workload
from oracle.pyoracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
N, SEED, STEPS, WARMUP = 4096, 11, 5, 3
SIZES = dict(n_routes_v4=4000, n_acl=300, n_nat=32)
NAMES = ("done", "sample_index", "sample_out", "sample_frames", "stats")
FULL_ONLY = ("roofline", "with_meta", "flow_table", "nat_portfw", "nat_masquerade", "nat_mixed",
             "host_inclusive", "host_inclusive_mpps", "cpu_baseline")


def _bench_module():
    spec = util.spec_from_file_location("bench_mod", BENCH)
    bench = util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


@pytest.fixture(scope="module")
def expected():
    """The workload `bench.py --config 2 --packets N --seed SEED` builds on rank
    0, and the oracle's result for it."""
    w = Workload(2, N, seed=shard_seed(SEED, 0), layout="dpdk", **SIZES)
    buf = w.fresh_buf()
    out = Oracle(w.tables).process(buf, w.inp)
    return w, buf, out


def _check_dump(bench, d, w, buf, out, steps):
    got = {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    assert np.array_equal(got["done"], out["done"].astype(np.float32))
    idx = got["sample_index"].astype(np.int64)
    assert len(idx) == min(N, bench.DUMP_SAMPLE) and np.all(np.diff(idx) > 0) and idx[-1] < N
    for j, f in enumerate(("off", "len", "done", "acl", "oif", "meta_flags")):
        assert np.array_equal(got["sample_out"][:, j], out[f][idx].astype(np.float64)), f
    deliv = 0
    for r, i in enumerate(idx):
        o, l = int(out["off"][i]), min(int(out["len"][i]), bench.DUMP_FRAME)
        want = np.zeros(bench.DUMP_FRAME, dtype=np.float32)
        if out["done"][i] == A.DONE["Delivered"]:
            want[:l] = buf[o:o + l]
            deliv += 1
        assert np.array_equal(got["sample_frames"][r], want), f"frame of packet {i}"
    assert deliv > len(idx) // 4
    assert np.array_equal(got["stats"], steps * np.bincount(out["done"], minlength=A.DONE_COUNT))


def test_dump_outputs_files(expected, tmp_path):
    w, buf, out = expected
    bench = _bench_module()
    stats = np.bincount(out["done"], minlength=A.DONE_COUNT).astype(np.int64)
    padded = np.concatenate([buf, np.zeros(-len(buf) % 256, dtype=np.uint8)])
    for _ in range(2):  # the same files whatever the directory held
        bench.dump_outputs(str(tmp_path / "d"), SEED, padded, len(buf), out, stats)
    _check_dump(bench, str(tmp_path / "d"), w, buf, out, 1)


def test_steps_and_warmup_validated():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--launch-probe"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_gpu_plain_run_dumps_the_last_step(expected, tmp_path):
    w, buf, out = expected
    bb = (w.buf.nbytes + 255) & ~255
    d = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--packets", str(N), "--seed", str(SEED), "--routes-v4",
                        str(SIZES["n_routes_v4"]), "--acl", str(SIZES["n_acl"]), "--nat",
                        str(SIZES["n_nat"]), "--staged-bytes", str(2 * bb), "--dump-outputs", d],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["n_gpus"] == 1
    assert res["unit"] == "Mpps" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(N / res["ms_per_step"] / 1e3, rel=1e-2)
    assert sum(res["done_histogram"].values()) == STEPS * N
    assert not [k for k in FULL_ONLY if k in res]
    _check_dump(_bench_module(), d, w, buf, out, STEPS)
