"""world_size-2 gloo tests of the N>1 path's host logic: contiguous image sharding, the single end-of-run gather
of typed (boxes, scores, tokens) records, and bench.py's real world=2 control flow (with its --stub model: no GPU
here; the same branch runs with the HIP model and two ranks on GPU 0 in tests/test_gpu_dist.py)."""
import os
import socket

import numpy as np


def _fake_forward(img_id, P, T):
    rng = np.random.default_rng(img_id)
    k = int(rng.integers(0, P + 1))
    return (rng.standard_normal((k, 4)).astype(np.float32), np.sort(rng.standard_normal(k).astype(np.float32))[::-1].copy(),
            rng.integers(1, 10499, (k, T)).astype(np.int32))


def _worker(rank, world, port, n_images, P, T, q):
    import torch.distributed as dist
    from densecap_amd import dist as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = D.shard_range(n_images, world, rank)
    results = [_fake_forward(i, P, T) for i in range(lo, hi)]
    per = (n_images + world - 1) // world
    while len(results) < per:                      # pad the last shard so gather shapes agree
        results.append((np.zeros((0, 4), np.float32), np.zeros((0,), np.float32), np.zeros((0, T), np.int32)))
    dist.barrier()
    out = D.gather_records(dist, results, P, T, rank, world)      # ONE collective: typed records, K inside
    if rank == 0:
        flat = [r for shard in out for r in shard][:n_images]
        ok = True
        for i, (b, s, t) in enumerate(flat):
            eb, es, et = _fake_forward(i, P, T)
            ok &= np.array_equal(b, eb) and np.array_equal(s, es) and np.array_equal(t, et)
        q.put(bool(ok))
    dist.destroy_process_group()


def test_shard_range_covers_all_images():
    from densecap_amd.dist import shard_range
    for n, w in [(512, 8), (7, 2), (3, 4), (1, 1), (64, 8)]:
        seen = []
        for r in range(w):
            lo, hi = shard_range(n, w, r)
            seen += list(range(lo, hi))
        assert seen == list(range(n))
    assert shard_range(512, 8, 3) == (192, 256)    # BASELINE config 4: 64 images per GPU


def test_gather_world2_gloo():
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, 7, 20, 15, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert q.get(timeout=5) is True


def test_record_pack_roundtrip_and_layout():
    """Typed record: {int32 K,T,P,0; f32 boxes[P][4]; f32 scores[P]; int32 tokens[P][T]} -- the layout comm.hip sends."""
    from densecap_amd import dist as D
    P, T = 9, 4
    res = [_fake_forward(i, P, T) for i in range(5)] + [(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros((0, T), np.int32))]
    buf = D.pack_records(res, P, T)
    assert buf.dtype == np.uint8 and buf.shape == (6, 16 + P * (16 + 4 + 4 * T))
    k0 = len(res[0][0])
    assert tuple(buf[0, :16].view(np.int32)) == (k0, T, P, 0)
    assert buf[0, 16 + 20 * P:16 + 20 * P + 4].view(np.int32)[0] == (res[0][2][0, 0] if k0 else 0)    # tokens stay int32
    for (b, s, t), (b2, s2, t2) in zip(res, D.unpack_records(buf)):
        np.testing.assert_array_equal(b, b2); np.testing.assert_array_equal(s, s2); np.testing.assert_array_equal(t, t2)
        assert t2.dtype == np.int32
    import pytest
    with pytest.raises(ValueError):
        D.pack_records([(np.zeros((P + 1, 4), np.float32), np.zeros(P + 1, np.float32), np.zeros((P + 1, T), np.int32))], P, T)


def test_bench_world2_branch_runs_under_gloo_with_stub_model():
    """bench.py's world>1 branch end to end (torch.distributed.run, 2 ranks, gloo, --stub model): one JSON line from
    rank 0, n_gpus = 2, the gather delivered both shards."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                        "--gpus", "2", "--stub", "--dist-backend", "gloo", "--steps", "4", "--warmup", "1",
                        "--repeats", "3", "--proposals", "50"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak" and d["data"] == "stub"
    assert d["config"]["total_output_boxes"] > 0 and len(d["repeats"]["images_per_s"]) == 3
    assert abs(d["value"] - 2 * 4 / (d["ms_per_step"] * 4e-3)) < 1e-6 * d["value"]


def test_bench_line_contract_single_process_stub():
    """The one JSON line bench.py prints carries every key of the driver's contract (checked without a GPU through the
    --stub model; the roofline / cpu_baseline objects need the device and are checked in tests/test_gpu_dist.py)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--stub", "--steps", "3", "--warmup", "1",
                        "--repeats", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "images/s" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32"
    assert "workload" in d["config"] and "model" not in d["config"]


def test_bench_plain_run_times_steps_once_and_dumps_the_last_step(tmp_path):
    """Without --full: ONE timed region of exactly --steps steps (no repeats, no sustained leg), ms_per_step is its time per
    step, and --dump-outputs writes the last step's arrays in float32 -- the same bytes on a second run with the same arguments."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--stub", "--steps", "5", "--warmup", "2",
                            "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        out.append(json.loads(lines[0]))
    d = out[0]
    assert d["steps"] == 5 and d["warmup"] == 2 and d["repeats"]["n"] == 1 and d["sustained"] is None
    assert abs(d["ms_per_step"] - 1e3 * d["repeats"]["timed_seconds_total"] / 5) < 1e-6 * d["ms_per_step"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    arrays = {}
    for name in ("boxes", "scores", "tokens", "boxes_per_image"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a, b), name
        arrays[name] = a
    k = int(arrays["boxes_per_image"][0])
    assert arrays["boxes"].shape == (k, 4) and arrays["scores"].shape == (k,) and arrays["tokens"].shape == (k, 15)


def _run_stub_bench(world, extra, timeout=600):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, OMP_NUM_THREADS="1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                        "--gpus", str(world), "--stub", "--dist-backend", "gloo", "--steps", "5", "--warmup", "1",
                        "--repeats", "2", "--proposals", "40"] + extra, capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    return json.loads(lines[0]), p.stderr


def test_bench_world8_control_flow_under_gloo():
    """The driver's 8-GPU launch, on CPU: 8 ranks, the lane choice broadcast from rank 0 (the stub's per-rank trial
    picks a different winner on every rank), the communicator-style carrier (--gather abi -> StubComm), the gather's
    [rank][image] order checked record by record against the global image ids, max-over-ranks time, one JSON line."""
    d, err = _run_stub_bench(8, ["--full", "--gather", "abi", "--stub-rank0-leg-seconds", "3"])
    # teardown hygiene (round-5 verdict, weak #10): the process group is destroyed on EVERY rank before rank 0's own legs (the
    # serial roofline pass, the CPU baseline, the counter passes: stood in for by a 3 s sleep) -- ranks >= 1 are gone by then,
    # nobody waits in a closing barrier under the collective watchdog
    import re
    gone = {int(r): float(t) for r, t in re.findall(r"bench.py\[rank (\d+)\]: process group destroyed t=([0-9.]+)", err)}
    begin = float(re.search(r"own legs begin t=([0-9.]+)", err).group(1))
    end = float(re.search(r"own legs end t=([0-9.]+)", err).group(1))
    assert sorted(gone) == list(range(8)) and end - begin >= 2.9
    assert gone[0] <= begin and all(gone[r] < begin + 1.0 for r in range(1, 8)), "ranks >= 1 must leave when rank 0's own legs begin"
    assert d["n_gpus"] == 8 and d["steps"] == 5 and d["scaling"] == "weak" and d["data"] == "stub"
    assert d["config"]["gather"].startswith("dc_gather_results") and d["config"]["gather_order_verified"] is True
    assert d["lanes"] == 2            # rank 0's trial {2: 102, 3: 100, 4: 101}; rank 1 alone would pick 4 (StubModel.autotuneLanes)
    assert d["sustained"]["images"] % (8 * 5) == 0 and d["sustained"]["images_per_s"] > 0
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    # self-diagnosing first run on a real node: every rank's own rate and the exact shard / byte table are in the line
    assert len(d["per_rank_images_per_s"]) == 8 and all(v > 0 for v in d["per_rank_images_per_s"])
    st = d["config"]["shard_table"]
    assert st["world"] == 8 and st["images_per_gpu"] == 5 and [x["global_images"] for x in st["shards"]][3] == [15, 20]
    rb = 16 + 40 * (16 + 4 + 4 * 15)              # --proposals 40 in the stub runs
    assert st["gather"]["record_bytes"] == rb and st["gather"]["block_bytes_per_rank"] == 5 * rb
    assert [(p["peer"], p["offset"]) for p in st["gather"]["rank0_posts"]] == [(p, p * 5 * rb) for p in range(1, 8)]
    assert st["gather"]["total_payload_bytes"] == 7 * 5 * rb and len(st["gather"]["peer_posts"]) == 7


def test_bench_dry_run_prints_the_shard_table_without_ranks():
    """`bench.py --gpus 8 --dry-run`: what the 8-GPU run of BASELINE configs[3] (512 images, 64 per GPU) will post, with no
    GPU, no torch.distributed and no ranks -- so that a driver with an 8-GPU node can check its first run against it."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-run"], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["dry_run"] is True and d["world"] == 8 and d["total_images_per_region"] == 512
    assert d["shards"][7] == {"rank": 7, "global_images": [448, 512]}
    g = d["gather"]
    assert g["record_bytes"] == 80016 and g["block_bytes_per_rank"] == 64 * 80016
    assert g["handshake"]["messages"] == 14 and g["total_payload_bytes"] == 7 * 64 * 80016
    assert all(p["op"] == "ncclSend" and p["peer"] == 0 and p["bytes"] == 64 * 80016 for p in g["peer_posts"])


def test_bench_world8_carrier_failure_falls_back_on_every_rank():
    """A carrier that cannot be created on ONE rank (librccl missing, ncclCommInitRank refused) must be dropped by ALL
    ranks together (all_ranks_ok) -- otherwise the job deadlocks with some ranks in the communicator and others in
    torch.distributed.  (A rank that dies INSIDE a collective cannot be recovered by anyone; not modelled.)"""
    d, err = _run_stub_bench(8, ["--gather", "abi", "--stub-comm-fail", "create:5"])
    assert d["config"]["gather"].startswith("torch.distributed.gather") and "dc_gather_results" in d["config"]["gather"]
    assert d["config"]["gather_order_verified"] is True and "WARNING" in err
