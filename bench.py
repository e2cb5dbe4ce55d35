#!/usr/bin/env python3
"""bench.py -- images/s of the densecap hot path on MI355X (BASELINE.json metric).

One "step" = DenseCapModel:forward_test on ONE synthetic 720x600 image with 1000 proposals
(BASELINE.json configs[1]): VGG-16 trunk -> RPN + NMS -> bilinear RoI pooling -> fc6/fc7 ->
heads -> greedy LSTM decode (T=15, V=10497) -> final NMS.  Images are resident in HBM before
the timed region; results (boxes, scores, tokens) come back to the host inside it.

Timed region = exactly K steps between barrier + device sync on both sides, max over ranks.  A plain run
(`--steps K --warmup W`) sets up, picks the schedule by an untimed trial, warms up with W steps, times ONE
region of K steps, writes the last step's outputs if `--dump-outputs DIR` is given and prints the line.
`--full` adds everything else: the region is repeated `--repeats` times (7) and the MEDIAN repeat is
reported, plus the sustained leg, the secondary legs, the roofline passes and the CPU baseline.

N GPUs: one process per GPU (torch.distributed), images sharded contiguously, weak scaling (K images
per GPU), ONE gather of the typed (boxes,scores,tokens) records on rank 0 at the end of each timed
region: dc_gather_results of the C ABI (RCCL send/recv over xGMI) or, with --gather torch, one
torch.distributed gather of the same packed records.  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 2.4 GHz
HBM_PEAK_GBPS = 8000.0
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16)
PMC_PROFILE = os.path.join("profiles", "r06_pmc_summary.json")
PARITY_REPORT = os.path.join("profiles", "r06_parity_report.json")
DISTINCT_IMAGES = 64          # synthetic images made per rank (BASELINE configs[3]: 64 per GPU); larger --steps repeat them

VGG = [(3, 64, 0), (64, 64, 1), (64, 128, 0), (128, 128, 1), (128, 256, 0), (256, 256, 0), (256, 256, 1),
       (256, 512, 0), (512, 512, 0), (512, 512, 1), (512, 512, 0), (512, 512, 0), (512, 512, 0)]


def stage_gflop(H, W, P, T, V, k=12, R=256, D=4096, E=512, Hd=512):
    """Algorithmic GFLOP (2 x MAC) per image and stage -- SURVEY.md 8(d)."""
    h, w, trunk = H, W, 0.0
    for cin, cout, pool in VGG:
        trunk += 2.0 * h * w * cin * cout * 9
        if pool:
            h, w = (h + 1) // 2, (w + 1) // 2
    rpn = 2.0 * h * w * (512 * R * 9 + R * 6 * k)
    fc = 2.0 * P * (512 * 49 * D + D * D)
    # encoder + step-0 gates + T x (h.Wh + vocabulary projection); the discarded step-0 projection is not computed
    lm = 2.0 * P * (D * E + E * 4 * Hd + T * Hd * 4 * Hd + T * Hd * (V + 1))
    return {"vgg16_trunk": trunk / 1e9, "rpn_conv_heads_decode": rpn / 1e9, "fc6_fc7": fc / 1e9, "lstm_decode": lm / 1e9}


def mfma_family_bytes(H, W, P, T, V, k=12, R=256, D=4096, E=512, Hd=512):
    """Algorithmic HBM bytes of the MFMA contraction family per image (operands read once + result written once per
    launch, fp32): the denominator `roofline.traffic` is judged against.  Returns (bytes per image, launches per image)."""
    h, w, total, launches = H, W, 0.0, 0
    for i, (cin, cout, pool) in enumerate(VGG):
        oh, ow = ((h + 1) // 2, (w + 1) // 2) if pool else (h, w)
        if i > 0:                      # conv1_1 is not a member of the family (its own kernel)
            total += 4.0 * (h * w * cin + cout * 9 * cin + oh * ow * cout)
            launches += 1
        h, w = oh, ow
    total += 4.0 * (h * w * 512 + R * 9 * 512 + h * w * R); launches += 1            # RPN conv
    total += 4.0 * (h * w * R + 6 * k * R + h * w * 6 * k); launches += 1            # fused 1x1 heads
    total += 4.0 * (P * 49 * 512 + D * 49 * 512 + P * D); launches += 1              # fc6
    total += 4.0 * (P * D + D * D + P * D); launches += 1                            # fc7
    total += 4.0 * (P * D + E * D + P * E); launches += 1                            # LM encoder
    total += 4.0 * (P * E + 4 * Hd * E + P * 4 * Hd); launches += 1                  # image step gates
    total += 4.0 * (P * Hd + 4 * Hd * Hd + P * 4 * Hd); launches += 1                # h0.Wh
    v1pad = (V + 1 + 63) // 64 * 64
    step = 4.0 * (P * Hd + (v1pad + 4 * Hd) * Hd + P * 4 * Hd + 2 * P * (v1pad // 32))   # [Wout; Wh] panel, gates out, arg-max partials (value + column per row and 32-column half)
    total += (T - 1) * step; launches += T - 1
    total += 4.0 * (P * Hd + (V + 1) * Hd + 2 * P * (v1pad // 32)); launches += 1    # last step: arg-max only
    return total, launches


def record_bytes(P, T):
    """One image's record in dc_gather_results: {K, T, capacity, 0; boxes[P][4]; scores[P]; int32 tokens[P][T]} (comm.hip)."""
    return 16 + P * (16 + 4 + 4 * T)


def shard_table(world, K, P, T):
    """What an N-GPU run of this file does, without running it: rank r owns global images [r*K, (r+1)*K) and the ONE
    gather per timed region posts, inside one RCCL group, world-1 receives on rank 0 and one send on every peer."""
    rb = record_bytes(P, T)
    block = rb * K
    return {
        "world": world, "images_per_gpu": K, "total_images_per_region": world * K,
        "shards": [{"rank": r, "global_images": [r * K, (r + 1) * K]} for r in range(world)],
        "gather": {
            "carrier": "dc_gather_results (RCCL ncclSend/ncclRecv in one group, include/densecap.h)",
            "record_bytes": rb, "block_bytes_per_rank": block,
            "handshake": {"peer_to_rank0_bytes": 16, "rank0_to_peer_bytes": 16, "messages": 2 * (world - 1)},
            "rank0_posts": [{"op": "ncclRecv", "peer": p, "bytes": block, "offset": block * p} for p in range(1, world)],
            "peer_posts": [{"rank": p, "op": "ncclSend", "peer": 0, "bytes": block} for p in range(1, world)],
            "total_payload_bytes": block * (world - 1),
            "unpack_order": "gathered[r * images_per_gpu + i] = image i of rank r"},
    }


class GpuSampler:
    """Polls the GPU's shader clock and power while a leg runs (sysfs: pp_dpm_sclk's active level and hwmon
    power1_average/power1_input; `rocm-smi --json` when sysfs has neither).  Means over the window go into the line so a
    reader can tell a sub-second burst at boost clocks from the sustained state."""

    def __init__(self, device_index=0, period=0.2):
        import glob
        import threading
        self.period = period
        self.sclk, self.power = [], []
        self.source = None
        self._stop = threading.Event()
        self._thread = None
        cards = []
        for c in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
            if os.path.exists(os.path.join(c, "device", "pp_dpm_sclk")):
                cards.append(c)
        want = None
        try:
            import torch
            bus = getattr(torch.cuda.get_device_properties(device_index), "pci_bus_id", None)
            if isinstance(bus, int):
                want = "%02x:" % bus
        except Exception:
            pass
        self.card = None
        for c in cards:
            if want and want in os.path.realpath(os.path.join(c, "device")):
                self.card = c
        if self.card is None and cards:
            self.card = cards[min(device_index, len(cards) - 1)]
        self.device_index = device_index

    def _read_sysfs(self):
        import glob
        mhz = watts = None
        try:
            for line in open(os.path.join(self.card, "device", "pp_dpm_sclk")):
                if "*" in line:
                    mhz = float(line.split(":")[1].strip().lower().replace("mhz", "").replace("*", "").strip())
        except Exception:
            pass
        for name in ("power1_average", "power1_input"):
            for f in glob.glob(os.path.join(self.card, "device", "hwmon", "hwmon*", name)):
                try:
                    watts = float(open(f).read().strip()) / 1e6
                    break
                except Exception:
                    pass
            if watts is not None:
                break
        return mhz, watts

    def _read_smi(self):
        try:
            o = subprocess.run(["rocm-smi", "-d", str(self.device_index), "--showclocks", "--showpower", "--json"],
                               capture_output=True, text=True, timeout=5).stdout
            d = json.loads(o)
            card = next(iter(d.values()))
            mhz = watts = None
            for k, v in card.items():
                kl = k.lower()
                if "sclk" in kl and "clock" in kl and mhz is None:
                    mhz = float(str(v).strip("()").lower().replace("mhz", ""))
                if "power" in kl and "(w)" in kl and watts is None:
                    watts = float(v)
            return mhz, watts
        except Exception:
            return None, None

    def _loop(self):
        while not self._stop.is_set():
            mhz, watts = self._read_sysfs() if self.card else (None, None)
            src = "sysfs"
            if mhz is None and watts is None:
                mhz, watts = self._read_smi()
                src = "rocm-smi"
            if mhz is not None or watts is not None:
                self.source = src
            if mhz is not None:
                self.sclk.append(mhz)
            if watts is not None:
                self.power.append(watts)
            self._stop.wait(self.period)

    def start(self):
        import threading
        self._thread = threading.Thread(target=self._loop, daemon=True)
        self._thread.start()
        return self

    def stop(self):
        self._stop.set()
        if self._thread is not None:
            self._thread.join(10)
        mean = lambda v: (sum(v) / len(v)) if v else None
        return {"sclk_mhz_mean": mean(self.sclk), "sclk_mhz_min": min(self.sclk) if self.sclk else None,
                "power_w_mean": mean(self.power), "samples": max(len(self.sclk), len(self.power)), "source": self.source}


class StubModel:
    """CPU stand-in with the product model's batch interface (bench.py --stub): lets the multi-rank control flow of this
    file (sharding, warm-up, barriers, gather, max-over-ranks timing, JSON) run under gloo without a GPU.  Its numbers
    are not measurements (the line says "data": "stub")."""
    seq_length = 15

    def __init__(self, P):
        self.P = P

    def setLanes(self, n):
        return self

    def forward_batch_device(self, imgs, n, H, W):
        import numpy as np
        out = []
        for i in range(n):
            rng = np.random.default_rng(int(imgs[i]))
            k = int(rng.integers(1, self.P + 1))
            out.append((rng.standard_normal((k, 4)).astype(np.float32),
                        np.sort(rng.standard_normal(k).astype(np.float32))[::-1].copy(),
                        rng.integers(1, 10499, (k, 15)).astype(np.int32)))
        return out

    def autotuneLanes(self, imgs, n, H, W, candidates=(2, 3, 4), reps=2):
        # every rank "measures" another winner: the job-wide choice must be rank 0's (broadcast in main)
        rank = int(os.environ.get("RANK", "0"))
        return {c: 100.0 + ((c + rank) % 3) for c in candidates}

    def stage_times(self):
        return {}

    def mfma_profile(self, reset=0):
        return dict(launches=0, ms=0.0, flops=0.0)


class StubComm:
    """Stand-in for densecap_amd.dist.Comm under --stub --gather abi: carries the records over torch.distributed like
    gather_records, and can be told to fail at creation on one rank so that the all-ranks fallback of main() runs on CPU."""

    def __init__(self, dist, rank, world, fail_rank=-1, fail_at="never"):
        self.dist, self.rank, self.world, self.fail_rank, self.fail_at = dist, rank, world, fail_rank, fail_at
        if fail_at == "create" and rank == fail_rank:
            raise RuntimeError("stub communicator refused on rank %d" % rank)

    def gather(self, results, P, T):
        from densecap_amd import dist as D
        return D.gather_records(self.dist, results, P, T, self.rank, self.world)

    transport = "stub carrier over torch.distributed"

    def close(self):
        pass


def dump_outputs(path, records):
    """Writes what the timed path handed back for its last step -- the (boxes, scores, token ids) record of every rank's last
    image of the last timed region, in rank order -- as float32 .npy files (token ids < 2^24 are exact).  Rows of all ranks
    are concatenated; boxes_per_image[r] is rank r's row count."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {"boxes": np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b, _, _ in records]),
              "scores": np.concatenate([np.asarray(s, np.float32).reshape(-1) for _, s, _ in records]),
              "tokens": np.concatenate([np.asarray(t) for _, _, t in records]).astype(np.float32),
              "boxes_per_image": np.array([len(b) for b, _, _ in records], np.float32)}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None



def measure_traffic_live(args, timeout_s=170):
    """HBM bytes per MFMA launch and MFMA-pipe utilisation, measured by THIS run: child passes of this command on one lane
    (per-kernel counters need kernels that do not overlap) under `rocprofv3 --kernel-trace --pmc <counters>` -- FETCH_SIZE,
    WRITE_SIZE and the MFMA-busy pair in SEPARATE passes, nothing else traced, as /opt/skills/guides/MI355X_MICROARCH.md
    prescribes -- summed over the dispatches of the mfma_gemm_* family exactly as tools/pmc_summary.py sums the committed passes:
    traffic = (2 x FETCH_SIZE + WRITE_SIZE) KB x 1024 / launches (FETCH_SIZE counts 32-byte requests as if they were 64 on
    gfx950: the guide's x2 for wide coalesced reads); utilisation = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024
    SIMDs), for the family and for its convolution kernels alone (the VGG-16 trunk + the RPN conv: CONV = true instantiations).
    Returns a dict or raises; never called under a profiler or from a child pass."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rp):
        raise RuntimeError("rocprofv3 not found")
    env = dict(os.environ, TMPDIR="/tmp", DC_BENCH_CHILD="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def is_conv(name):                 # mfma_gemm_ks/sk_kernel<true>, mfma_gemm_v2_mixed_kernel<true, ..>, mfma_gemm_v2_kernel<TM, TN, true, ..>, mfma_gemm_bf3_128_kernel<true, ..>
        a = name.split("<", 1)[1].split(",") if "<" in name else []
        a = [x.strip(" >") for x in a]
        return bool(a) and (a[0] == "true" or (name.startswith("mfma_gemm_v2_kernel") and len(a) > 2 and a[2] == "true"))
    per = {}
    t0 = time.perf_counter()
    for tag, counters in (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]), ("mfma", ["SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE"])):
        out = tempfile.mkdtemp(prefix="dc_pmc_", dir="/tmp")
        try:
            cmd = [rp, "--kernel-trace", "--pmc"] + counters + ["--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable,
                   os.path.abspath(__file__), "--lanes", "1", "--group", "1", "--steps", "3", "--warmup", "1", "--repeats", "1",
                   "--height", str(args.height), "--width", str(args.width), "--proposals", str(args.proposals),
                   "--math-mode", str(args.math_mode), "--no-cpu-baseline", "--no-alt-pass", "--no-host-input-leg",
                   "--sustain-seconds", "0", "--no-settle", "--no-split-leg", "--no-traffic-leg", "--gather", "torch"]
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=True)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                raise RuntimeError("no counter file from the %s pass" % tag)
            acc = {c: [0.0, 0.0, 0.0, 0.0] for c in counters}        # [family, conv kernels, RoI pooling, NMS kernels]
            disp, disp_roi, disp_nms = set(), set(), set()
            for r in csv.DictReader(open(files[0])):
                name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                if r["Counter_Name"] not in acc:
                    continue
                v = float(r["Counter_Value"])
                if name.startswith("mfma_gemm"):
                    acc[r["Counter_Name"]][0] += v
                    if is_conv(name):
                        acc[r["Counter_Name"]][1] += v
                    disp.add(r["Dispatch_Id"])
                elif name.startswith("bilinear_roi_pool"):
                    acc[r["Counter_Name"]][2] += v
                    disp_roi.add(r["Dispatch_Id"])
                elif name.startswith("nms_"):
                    acc[r["Counter_Name"]][3] += v
                    disp_nms.add(r["Dispatch_Id"])
            if not disp:
                raise RuntimeError("no mfma_gemm dispatch in the %s pass" % tag)
            per[tag] = (acc, len(disp))
            per[tag + "_n"] = (len(disp_roi), len(disp_nms))
        finally:
            shutil.rmtree(out, ignore_errors=True)
    (fa, nf), (wa, nw), (ma, nm) = per["fetch"], per["write"], per["mfma"]
    f, w = fa["FETCH_SIZE"][0], wa["WRITE_SIZE"][0]
    busy, gui = ma["SQ_VALU_MFMA_BUSY_CYCLES"], ma["GRBM_GUI_ACTIVE"]
    util = lambda i: busy[i] / (gui[i] / 8.0 * 1024.0) if gui[i] > 0 else None
    nroi, nnms = per["fetch_n"]
    nimg = max(nroi, 1)                                        # one RoI-pooling launch per image on this schedule
    hbm_stage = {}
    if nroi:
        hbm_stage["bilinear_roi_pool_kernel"] = {"fetch_kb_per_launch": fa["FETCH_SIZE"][2] / nroi, "write_kb_per_launch": wa["WRITE_SIZE"][2] / max(per["write_n"][0], 1),
                                                 "hbm_bytes_per_launch": (2.0 * fa["FETCH_SIZE"][2] / nroi + wa["WRITE_SIZE"][2] / max(per["write_n"][0], 1)) * 1024.0}
    if nnms:
        hbm_stage["nms_kernels"] = {"launches_per_image": nnms / nimg,
                                    "hbm_bytes_per_image": (2.0 * fa["FETCH_SIZE"][3] + wa["WRITE_SIZE"][3]) * 1024.0 / nimg}
    return {"hbm_bytes_per_launch": (2.0 * f / nf + w / nw) * 1024.0, "fetch_kb_per_launch": f / nf, "write_kb_per_launch": w / nw,
            "launches_counted": nf, "mfma_util_family": util(0), "mfma_util_conv_kernels": util(1), "hbm_stage_kernels": hbm_stage,
            "seconds": time.perf_counter() - t0,
            "how": "live: three child passes of this command (--lanes 1 --group 1 --steps 3) under rocprofv3 --kernel-trace --pmc "
                   "FETCH_SIZE | WRITE_SIZE | SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE, mfma_gemm_* dispatches: (2 x FETCH_SIZE + "
                   "WRITE_SIZE) KB x 1024 / launches; MFMA busy cycles / (GUI-active cycles / 8 XCDs x 1024 SIMDs), at the "
                   "profiler's clocks (2.0-2.3 GHz), for the family and for its convolution kernels (VGG-16 trunk + RPN conv)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64, help="images per timed region and GPU (BASELINE configs[3] shards 64 per GPU)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed regions of --steps steps each; the median is reported (default 1; 7 with --full)")
    ap.add_argument("--sustain-seconds", type=float, default=None,
                    help="length of the sustained leg (back-to-back timed regions with clock/power sampling); 0 = skip "
                         "(default 0; 10 with --full)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: warm-up until stable, 7 repeats, the sustained leg, the H2D-inclusive "
                         "legs, the caption-order and split-bf16 legs, the serial roofline pass, the other BASELINE configs, the "
                         "live counter passes, the CPU baseline and the in-run parity check.  Without it a run sets up, warms up, "
                         "times --steps steps once and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step (boxes, scores, token ids of every "
                         "rank's last image) to DIR/<name>.npy in float32")
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--proposals", type=int, default=1000)
    ap.add_argument("--lanes", type=int, default=0,
                    help="streams images are pipelined over (1 = serial, 0 = pick 2/3/4 by an untimed trial before the timed region)")
    ap.add_argument("--group", type=int, default=-1,
                    help="images per group inside a lane (dc_set_group, a scheduling knob: results are bit-identical): 1 = every image "
                         "on its own, 2..4 = the group's images share the dense launches, -1 (default) = pick 1 / 2 / 4 by an untimed trial")
    ap.add_argument("--plan-mode", type=int, default=-1, choices=[-1, 0, 1],
                    help="contraction planning: -1 follows --lanes (default), 0 = multi-lane planning even with --lanes 1 (profiler passes "
                         "that must see the kernels of the timed multi-lane schedule on one stream), 1 = single-image planning")
    ap.add_argument("--math-mode", type=int, default=0, choices=[0, 1],
                    help="dc_set_math_mode for the WHOLE run: 0 = fp32 MFMA (default, the headline), 1 = split-bf16 (opt-in mode; the line's "
                         "dtype / roofline then describe that mode and say so)")
    ap.add_argument("--caption-order", type=int, default=0, choices=[0, 1],
                    help="profiler / lab option, NOT the headline: 1 = every region of this run in the captions-after-the-final-NMS "
                         "schedule (dc_set_caption_order(1), what the CLIs run); the line says so in config.caption_order, counts the "
                         "language-model FLOPs of the decoded rows only and carries no value_captions_after_final_nms leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-alt-pass", action="store_true",
                    help="skip the secondary caption-order measurement (keeps rocprof kernel statistics to one workload)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for barriers / timing (gloo: ranks may share one GPU, or none with --stub)")
    ap.add_argument("--gather", default="auto", choices=["auto", "abi", "torch"],
                    help="carrier of the end-of-run gather: abi = dc_gather_results (RCCL), torch = torch.distributed.gather")
    ap.add_argument("--dry-run", action="store_true",
                    help="print the per-rank shard table and the exact RCCL byte counts an N-GPU run would post, then exit (no GPU, no ranks)")
    ap.add_argument("--no-host-input-leg", action="store_true", help="skip the H2D-inclusive legs (images in host memory)")
    ap.add_argument("--no-settle", action="store_true", help="skip the warm-up-until-stable regions (profiler passes)")
    ap.add_argument("--no-split-leg", action="store_true", help="skip the secondary split-bf16 measurement (value_split_bf16)")
    ap.add_argument("--no-traffic-leg", action="store_true",
                    help="skip the live HBM-traffic / MFMA-utilisation measurement (three rocprofv3 --pmc child passes of this command on one lane); "
                         "`roofline.traffic` is then quoted from the committed profile")
    ap.add_argument("--no-config-legs", action="store_true",
                    help="skip the short legs on the other BASELINE.json configs (`configs` in the line: configs[2] 32 x 300 proposals, "
                         "configs[4] 1080x720 / 2000 proposals, configs[0]'s 720x480 size)")
    ap.add_argument("--config-leg-seconds", type=float, default=2.0, help="timed seconds per configs leg and caption order")
    ap.add_argument("--stub", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--stub-rank0-leg-seconds", type=float, default=0.0, help=argparse.SUPPRESS)   # a stand-in for rank 0's own legs (teardown test)
    ap.add_argument("--stub-comm-fail", default="never:-1", help=argparse.SUPPRESS)   # "create:R": StubComm cannot be created on rank R
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 7 if args.full else 1
    if args.sustain_seconds is None:
        args.sustain_seconds = 10.0 if args.full else 0.0
    if not args.full:
        # a plain run does only what `value` needs: every secondary leg stays off
        args.no_settle = args.no_cpu_baseline = args.no_alt_pass = args.no_host_input_leg = True
        args.no_split_leg = args.no_traffic_leg = args.no_config_legs = True

    if args.dry_run:
        world = int(os.environ.get("WORLD_SIZE", args.gpus))
        print(json.dumps({"dry_run": True, "metric": "images/sec at 720x600, 1000 proposals", "n_gpus": world,
                          "config": {"height": args.height, "width": args.width, "proposals": args.proposals,
                                     "parallelism": "image-sharded x%d" % world},
                          **shard_table(world, args.steps, args.proposals, 15)}), flush=True)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # called directly with --gpus N: start one rank per GPU the way the driver does
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.execvp(sys.executable, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                   "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
                                   "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:])

    import numpy as np
    import torch  # device sync + torch.distributed; loaded first so one HIP runtime is shared

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # stdout carries ONE line, rank 0's JSON, and it is the LAST line: RCCL prints a version banner through C stdio when a
    # communicator is made (buffered, so it would surface after the JSON at exit).  Ranks other than 0 send their C-level
    # stdout to stderr from the start; rank 0 flushes C stdio before the line and closes stdout to C code after it.
    import ctypes
    _libc = ctypes.CDLL(None)
    if rank != 0:
        sys.stdout.flush(); _libc.fflush(None)
        os.dup2(2, 1)
    on_gpu = not args.stub
    # ranks may outnumber the visible GPUs only in the gloo configuration (two ranks on GPU 0 in the tests)
    ndev = torch.cuda.device_count() if on_gpu else 0
    device_index = local_rank % max(ndev, 1)
    if on_gpu and args.dist_backend == "nccl" and world > ndev:
        raise SystemExit("bench.py: %d ranks but %d GPUs visible (RCCL needs one GPU per rank)" % (world, ndev))
    if world > 1 or "WORLD_SIZE" in os.environ:
        # (a one-rank job started by torch.distributed.run still builds its process group: torch's RCCL and the library's
        # dlopen()ed librccl then live in one process, as they do in every rank of an N-GPU run)
        import torch.distributed as dist
        if on_gpu:
            torch.cuda.set_device(device_index)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group("gloo")
    else:
        dist = None
    gather_kind = args.gather
    if gather_kind == "auto":
        gather_kind = "abi" if (args.dist_backend == "nccl" and on_gpu) else "torch"
    coll_device = torch.device("cuda", device_index) if (args.dist_backend == "nccl" and on_gpu) else None

    H, W, P, K, Wm = args.height, args.width, args.proposals, args.steps, args.warmup
    T, V = 15, 10497
    n_img = max(K, Wm, args.lanes, 8, 1)                      # (>= dc_set_group's maximum: a whole group is resident even for --steps 4)
    n_distinct = min(n_img, DISTINCT_IMAGES)
    if on_gpu:
        from densecap_amd import DenseCapModel
        from densecap_amd._lib import check
        from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
        weights = make_synthetic_weights(seed=1234)           # V=10497, T=15 in checkpoint shapes
        model = DenseCapModel(weights, device=device_index)
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
        model.setLanes(args.lanes if args.lanes > 0 else 3)
        model.setGroup(max(args.group, 0))
        model.setMathMode(args.math_mode)
        if args.caption_order:
            model.setCaptionOrder(True)
            args.no_alt_pass = True
        ctx = model.ctx
        if args.plan_mode >= 0:
            check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"plan_mode", args.plan_mode), "dc_debug_set")
        # n_img images per rank resident in HBM: up to DISTINCT_IMAGES distinct ones (global image id = rank*n_img + i), repeated
        # in order beyond that, so that setup time does not grow with --steps
        host = np.stack([make_synthetic_image(H, W, rank * n_img + i) for i in range(n_distinct)])
        dev = ctx.empty((n_img,) + host.shape[1:])
        for i0 in range(0, n_img, n_distinct):
            nb_ = min(n_distinct, n_img - i0) * host[0].nbytes
            check(ctx.h, ctx.lib.dc_memcpy_h2d(ctx.h, ctypes.c_void_p(dev.ptr.value + i0 * host[0].nbytes), host.ctypes.data, nb_),
                  "dc_memcpy_h2d")
        imgs = dev.ptr

        def sync():
            check(ctx.h, ctx.lib.dc_synchronize(ctx.h), "dc_synchronize")
            torch.cuda.synchronize()
    else:
        model = StubModel(P)
        imgs = [rank * n_img + i for i in range(n_img)]

        def sync():
            pass

    def barrier():
        if dist is not None:
            dist.barrier()

    # ---- the path's single collective -------------------------------------------------------------------
    comm = None
    gather_note = None

    abandoned = []     # carriers stuck in a call that never returned: never closed, the process leaves through os._exit

    def guarded(fn, what, timeout=90.0):
        """Run a carrier call that has never executed on this kind of hardware before (RCCL point-to-point inside
        libdensecap_hip.so) in a daemon thread: a call that HANGS must cost the carrier, not the measurement.  Returns
        (result, error); error is an exception or a TimeoutError."""
        import threading
        box = {}

        def run():
            try:
                box["v"] = fn()
            except Exception as e:       # noqa: BLE001
                box["e"] = e
        th = threading.Thread(target=run, daemon=True)
        th.start()
        th.join(timeout)
        if th.is_alive():
            return None, TimeoutError("%s did not return within %.0f s" % (what, timeout))
        return box.get("v"), box.get("e")

    def all_ranks_ok(ok):
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=coll_device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    if dist is not None and gather_kind == "abi" and not on_gpu:
        fail_at, fail_rank = args.stub_comm_fail.split(":")
        err = None
        try:
            comm = StubComm(dist, rank, world, int(fail_rank), fail_at)
        except Exception as e:
            err = e
        if not all_ranks_ok(comm is not None):
            comm = None
            gather_note = "dc_gather_results unavailable (%s)" % (err if err is not None else "failed on another rank")
            print("bench.py[rank %d]: WARNING: %s -- gathering with torch.distributed.gather instead" % (rank, gather_note),
                  file=sys.stderr, flush=True)
    elif dist is not None and gather_kind == "abi":
        from densecap_amd import dist as D
        err = None
        idt = torch.zeros(128, dtype=torch.uint8)
        try:
            if rank == 0:
                idt = torch.frombuffer(bytearray(D.Comm.unique_id(ctx.lib)), dtype=torch.uint8).clone()
        except Exception as e:                               # e.g. librccl cannot be opened
            err = e
        idt = idt.to(coll_device) if coll_device is not None else idt
        dist.broadcast(idt, src=0)                       # rendezvous id of the RCCL communicator, out of band
        if all_ranks_ok(err is None):
            idb = bytes(idt.cpu().numpy().tobytes())
            comm, err = guarded(lambda: D.Comm(ctx, rank, world, idb, self_transport=(world == 1)),
                                "dc_comm_create (ncclCommInitRank)")
            if isinstance(err, TimeoutError):
                abandoned.append("dc_comm_create")
        if not all_ranks_ok(comm is not None):
            # The measurement must not be lost to the carrier: say so loudly and carry the same records over
            # torch.distributed instead (the line's config.gather records which carrier ran and why).
            if comm is not None:
                comm.close()
            comm = None
            gather_note = "dc_gather_results unavailable (%s)" % (err if err is not None else "failed on another rank")
            print("bench.py[rank %d]: WARNING: %s -- gathering with torch.distributed.gather instead" % (rank, gather_note),
                  file=sys.stderr, flush=True)

    if dist is None and on_gpu and gather_kind == "abi":
        # One GPU, no launcher: the end-of-region gather still runs, through the SAME carrier an N-GPU job uses --
        # dc_gather_results over an RCCL communicator of one rank, rank 0 sending its block to itself (DC_COMM_SELF_TRANSPORT).
        # Its first execution anywhere must not be the 8-GPU run's; a carrier that fails or hangs here costs the carrier only.
        from densecap_amd import dist as D
        comm, err = guarded(lambda: D.Comm(ctx, 0, 1, None, self_transport=True), "dc_comm_create (ncclCommInitRank, one rank)")
        if isinstance(err, TimeoutError):
            abandoned.append("dc_comm_create")
        if comm is None:
            gather_note = "dc_gather_results over RCCL unavailable at world 1 (%s)" % err
            print("bench.py: WARNING: %s -- results are taken as returned" % gather_note, file=sys.stderr, flush=True)

    def gather(results):
        from densecap_amd import dist as D
        if comm is not None:                 # (rebound to None below if the RCCL carrier turns out unusable)
            return comm.gather(results, P, model.seq_length)
        if dist is None:
            return [results]
        return D.gather_records(dist, results, P, model.seq_length, rank, world, device=coll_device)

    # ---- setup (not a step): lane workspaces, lane-count trial, warm-up incl. the collective ------------------
    lane_trials = None
    sched_trials = None
    group_fixed = args.group >= 0                            # --group given: the split-bf16 leg keeps it too
    if args.lanes <= 0 and args.group < 0 and on_gpu:
        # both scheduling knobs together (results are bit-identical for every pair): the best lane count depends on the group size
        # (the trial runs regions of exactly K images, the size of a timed region: with few images per region the best pair
        # depends on how the groups fall on the lanes -- 20 images are five groups of four on two lanes, three against two);
        # at most DISTINCT_IMAGES images, so that the trial's 24 regions stay a few seconds at any --steps
        sched_trials = model.autotuneSchedule(imgs, min(n_distinct, K), H, W)
        args.lanes, args.group = max(sched_trials, key=sched_trials.get)
        if dist is not None:
            lt = torch.tensor([args.lanes, args.group], dtype=torch.int32, device=coll_device)
            dist.broadcast(lt, src=0)
            args.lanes, args.group = int(lt[0].item()), int(lt[1].item())
        model.setLanes(args.lanes); model.setGroup(args.group)
    if args.lanes <= 0:
        # scheduling knob only (results are bit-identical for any lanes >= 2): which count overlaps best differs
        # between otherwise identical boxes, so it is chosen by a short untimed trial on this device
        lane_trials = model.autotuneLanes(imgs, min(n_img, 12), H, W)
        args.lanes = max(lane_trials, key=lane_trials.get)
        if dist is not None:
            # one setting for the whole job (a rank-local choice would still be valid, this keeps the line simple)
            lt = torch.tensor([args.lanes], dtype=torch.int32, device=coll_device)
            dist.broadcast(lt, src=0)
            args.lanes = int(lt.item())
            model.setLanes(args.lanes)
    group_trials = None
    if args.group < 0:
        args.group = 1
        if on_gpu and args.lanes != 1:
            # the same kind of knob as the lane count: images per group inside a lane (bit-identical results)
            group_trials = model.autotuneGroup(imgs, min(n_img, 16), H, W)
            args.group = max(group_trials, key=group_trials.get)
        if dist is not None:
            gt = torch.tensor([args.group], dtype=torch.int32, device=coll_device)
            dist.broadcast(gt, src=0)
            args.group = int(gt.item())
        if on_gpu:
            model.setGroup(args.group)
    if on_gpu and args.lanes == 1:
        # per-launch events from the first image on: the whole invocation stays on ONE stream (single-image mode would run
        # the un-timed setup / warm-up images with the two-stream decode and leave their kernels in a rocprofv3 trace)
        model.mfma_profile(reset=1)
    model.forward_batch_device(imgs, min(args.lanes, n_img), H, W)
    wres = model.forward_batch_device(imgs, max(Wm, 1), H, W)
    if dist is not None or comm is not None:
        # communicator / buffer setup of the first collective is not part of a step; a carrier that fails here is replaced
        warm = ([wres[0]] * K)[:K]
        if comm is not None:
            _, err = guarded(lambda: gather(warm), "dc_gather_results (warm-up)")
            stuck = isinstance(err, TimeoutError)
            if not (all_ranks_ok(err is None) if dist is not None else err is None):
                if stuck:
                    abandoned.append(comm)        # a thread is still inside it: never touch it again
                else:
                    comm.close()
                comm = None
                gather_note = "dc_gather_results failed in the warm-up (%s)" % (err if err is not None else "on another rank")
                print("bench.py[rank %d]: WARNING: %s -- gathering with torch.distributed.gather instead" % (rank, gather_note),
                      file=sys.stderr, flush=True)
        if comm is None and dist is not None:
            gather(warm)
    sync()
    # Warm-up until it IS warm (round-4 verdict: the first timed region of a fresh process ran at 134 images/s against 180 for
    # the other six -- W images do not bring the clocks up).  Untimed regions of K images repeat until two consecutive ones
    # agree within 2 % (at most 8); how many it took is in the line.
    warm_regions = []
    if on_gpu and not args.no_settle:
        prev = None
        for _ in range(8):
            barrier(); sync()
            w0 = time.perf_counter()
            model.forward_batch_device(imgs, K, H, W)
            sync()
            wt = time.perf_counter() - w0
            if dist is not None:
                tt = torch.tensor([wt], dtype=torch.float64, device=coll_device)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                wt = float(tt.item())
            warm_regions.append(K * world / wt)
            if prev is not None and abs(wt - prev) <= 0.02 * prev:
                break
            prev = wt
    if on_gpu and args.lanes == 1:
        model.mfma_profile(reset=1)      # HIP events around every MFMA launch during the timed regions

    # ---- timed regions ----------------------------------------------------------------------------------------
    elapsed_all, total_boxes, own_all = [], 0, []
    for rep in range(max(1, args.repeats)):
        barrier()
        sync()
        t0 = time.perf_counter()
        results = model.forward_batch_device(imgs, K, H, W)
        own_all.append(time.perf_counter() - t0)          # this rank's own shard, before the gather and the closing barrier
        gathered = gather(results)
        sync()
        barrier()
        elapsed = time.perf_counter() - t0
        if dist is not None:
            tt = torch.tensor([elapsed], dtype=torch.float64, device=coll_device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
        elapsed_all.append(elapsed)
        if rank == 0:
            total_boxes = int(sum(len(b) for shard in gathered for b, _, _ in shard))
            if dist is not None:
                assert len(gathered) == world and all(len(s) == K for s in gathered), "gather returned a wrong shape"
    gather_order_verified = None
    if rank == 0 and not on_gpu:
        # stub records are a function of the global image id: entry [r][i] must be image r*n_img + i of rank r's shard
        ref = StubModel(P)
        gather_order_verified = all(
            all(np.array_equal(x, y) for x, y in zip(gathered[r][i], ref.forward_batch_device([r * n_img + i], 1, H, W)[0]))
            for r in range(world) for i in range(K))
        assert gather_order_verified, "gather delivered records in a wrong order"
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, [shard[-1] for shard in gathered])
    host_enqueue_us = None
    if on_gpu:
        try:       # host time spent enqueueing one image of the last timed region (the N-GPU ceiling is 1 / this per rank)
            he, _ = model.debug_fetch("host_enqueue_us", (1,), np.int32)
            host_enqueue_us = int(he[0])
        except Exception:
            pass
    # --lanes 1: the per-launch events stay on (one stream for the whole invocation), but the counts that go with the timed
    # regions are read HERE -- the sustained leg below adds launches that K * repeats does not count
    prof_timed = model.mfma_profile(reset=0) if (on_gpu and args.lanes == 1) else None
    order = sorted(range(len(elapsed_all)), key=lambda i: elapsed_all[i])
    elapsed = elapsed_all[order[len(order) // 2]]          # median repeat
    nrep = len(elapsed_all)
    # per-rank rate of the median region (each rank's own shard, gather and closing barrier excluded): a slow GPU / NUMA
    # placement shows up here before it shows in the max-over-ranks time
    own_rate = K / max(own_all[order[len(order) // 2]], 1e-9)
    per_rank_rates = [own_rate]
    if dist is not None:
        tt = torch.tensor([own_rate], dtype=torch.float64, device=coll_device)
        allr = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(allr, tt)
        per_rank_rates = [float(t.item()) for t in allr]

    # ---- H2D-inclusive legs ("include H2D of the image"): the same K images (at most DISTINCT_IMAGES) in HOST
    # memory, pageable and pinned, through dc_forward_batch(imgs_on_device = 0).  `value` keeps inputs resident in HBM (the tier's rule); these
    # two figures say what the boundary delivers when it is handed host buffers.
    host_legs = None
    if on_gpu and dist is None and not args.no_host_input_leg:
        host_legs = {}
        pinned_t = torch.from_numpy(host[:K]).pin_memory()
        for kind, arr in (("pageable", host[:K]), ("pinned", pinned_t.numpy())):
            model.forward_batch(arr[:min(K, args.lanes)])
            sync()
            h0 = time.perf_counter()
            model.forward_batch(arr)
            sync()
            host_legs[kind] = len(arr) / (time.perf_counter() - h0)
        del pinned_t

    # ---- sustained leg: the same timed region back to back for >= --sustain-seconds, clocks and power sampled ---------
    # A 0.4 s region can ride boost clocks that a production loop never sees; this leg is what a long run delivers.
    sustained = None
    if args.stub:
        args.sustain_seconds = min(args.sustain_seconds, 0.2)      # control-flow runs only
    if args.sustain_seconds > 0:
        iters = max(2, int(args.sustain_seconds / max(elapsed, 1e-6) + 0.999))
        if dist is not None:
            it = torch.tensor([iters], dtype=torch.int32, device=coll_device)
            dist.broadcast(it, src=0)
            iters = int(it.item())
        sampler = GpuSampler(device_index).start() if (on_gpu and rank == 0) else None
        barrier()
        sync()
        s0 = time.perf_counter()
        for _ in range(iters):
            gather(model.forward_batch_device(imgs, K, H, W))
        sync()
        barrier()
        sdt = time.perf_counter() - s0
        if dist is not None:
            tt = torch.tensor([sdt], dtype=torch.float64, device=coll_device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            sdt = float(tt.item())
        sustained = {"images_per_s": world * K * iters / sdt, "seconds": sdt, "regions": iters, "images": world * K * iters}
        if sampler is not None:
            sustained.update(sampler.stop())
    prof = model.mfma_profile(reset=-1)
    if prof_timed is not None:
        prof = prof_timed
    stage = model.stage_times()

    # ---- every collective of the run is behind us: the process group goes away BEFORE rank 0's own legs ----------------
    # (round-5 verdict, weak #10: ranks >= 1 used to sit in the closing barrier -- with the nccl backend a spinning GPU kernel
    # under the 10-minute watchdog -- while rank 0 ran the serial roofline pass, the CPU baseline and the counter passes.)
    # Everything below is rank 0's alone and uses no collective; the other ranks leave here.
    had_dist = dist is not None
    carrier = ("dc_gather_results (%s)" % comm.transport) if comm is not None else None     # what carried the gathers of the timed regions
    if had_dist:
        if comm is not None and not abandoned:
            comm.close()
            comm = None
        dist.barrier()
        if abandoned:
            sys.stdout.flush(); sys.stderr.flush()
            os._exit(0)               # a carrier call never returned on this rank: no orderly teardown possible
        dist.destroy_process_group()
        dist = None
        print("bench.py[rank %d]: process group destroyed t=%.3f" % (rank, time.time()), file=sys.stderr, flush=True)
        if rank != 0:
            return
    if args.stub and args.stub_rank0_leg_seconds > 0:
        print("bench.py[rank 0]: own legs begin t=%.3f" % time.time(), file=sys.stderr, flush=True)
        time.sleep(args.stub_rank0_leg_seconds)
        print("bench.py[rank 0]: own legs end t=%.3f" % time.time(), file=sys.stderr, flush=True)

    # Secondary figure (not `value`): final NMS first, captions only for the surviving boxes -- bit-identical
    # outputs (tests/test_gpu_e2e.py::test_caption_order_is_output_invariant), less LSTM work.
    alt = None
    if on_gpu and not had_dist and not args.no_alt_pass:
        model.setCaptionOrder(True)
        # its own schedule (both knobs are pure scheduling here too: bit-identical results): the packed decode of a group of four
        # runs ~900 rows a launch where a single image has ~225, so the pair the reference order picked is not this order's best
        alt_sched, alt_trial = (args.lanes, args.group), None
        if args.lanes != 1 and not group_fixed:
            alt_trial = model.autotuneSchedule(imgs, min(n_distinct, K), H, W)
            alt_sched = max(alt_trial, key=alt_trial.get)
        model.setLanes(alt_sched[0]); model.setGroup(alt_sched[1])
        model.forward_batch_device(imgs, K, H, W)            # warm
        sync()
        alt_rates, alt_results = [], None
        for _ in range(5):
            sync()
            a0 = time.perf_counter()
            alt_results = model.forward_batch_device(imgs, K, H, W)
            sync()
            alt_rates.append(K / (time.perf_counter() - a0))
        model.setCaptionOrder(False)
        model.setLanes(args.lanes); model.setGroup(args.group)
        alt = {"images_per_s": sorted(alt_rates)[len(alt_rates) // 2], "regions": alt_rates, "lanes": alt_sched[0], "group": alt_sched[1],
               "trial": None if alt_trial is None else {"lanes%d_group%d" % k: v for k, v in alt_trial.items()},
               "rows_decoded_per_image": float(np.mean([len(b) for b, _, _ in alt_results])),
               # the SAME images as the last timed region of `value` (reference caption order): every array must be equal
               "identical": bool(len(alt_results) == len(results) and all(
                   np.array_equal(x, y) for a_, b_ in zip(alt_results, results) for x, y in zip(a_, b_)))}
    # Secondary figure (NOT `value`, fenced off from the fp32 headline): the same timed region in the opt-in split-bf16
    # arithmetic (dc_set_math_mode(1): operands as three bf16 planes, six partial products on the bf16 matrix cores, fp32
    # accumulate).  Its own roofline object prices it against the bf16 peak / 6.
    split = None
    if on_gpu and not had_dist and args.math_mode == 0 and not args.no_split_leg:
        model.setMathMode(1)
        model.forward_batch_device(imgs, K, H, W)            # warm (and clocks settle to this mode's power draw)
        sync()
        # images per group re-picked for this mode (its dense launches are shorter: the fp32 pick is not its best), untimed
        split_group, split_group_trial = args.group, None
        if args.lanes != 1 and not group_fixed:
            split_group_trial = {}
            for g in (1, 2, 4, 8):
                model.setGroup(g)
                model.forward_batch_device(imgs, K, H, W)
                sync()
                g0 = time.perf_counter()
                model.forward_batch_device(imgs, K, H, W)
                sync()
                split_group_trial[g] = K / (time.perf_counter() - g0)
            split_group = max(split_group_trial, key=split_group_trial.get)
            model.setGroup(split_group)
        rates, split_results = [], None
        for _ in range(3):
            sync()
            s0 = time.perf_counter()
            split_results = gather(model.forward_batch_device(imgs, K, H, W))[0]
            sync()
            rates.append(K / (time.perf_counter() - s0))
        # the same mode in the captions-after-the-final-NMS schedule (what the CLIs run with -math_mode 1): the two opt-in knobs
        # together, the highest rate the library delivers.  The alt leg's schedule; results compared with this leg's above.
        split_alt = None
        if alt is not None:
            model.setCaptionOrder(True)
            model.setLanes(alt["lanes"]); model.setGroup(alt["group"])
            model.forward_batch_device(imgs, K, H, W)
            sync()
            rates2, res2 = [], None
            for _ in range(3):
                sync()
                s0 = time.perf_counter()
                res2 = model.forward_batch_device(imgs, K, H, W)
                sync()
                rates2.append(K / (time.perf_counter() - s0))
            model.setCaptionOrder(False)
            model.setLanes(args.lanes)
            split_alt = {"images_per_s": sorted(rates2)[1], "regions": rates2, "lanes": alt["lanes"], "group": alt["group"],
                         "rows_decoded_per_image": float(np.mean([len(b) for b, _, _ in res2])),
                         "identical_to_the_reference_order_in_this_mode": bool(len(res2) == len(split_results) and all(
                             np.array_equal(x, y) for a_, b_ in zip(res2, split_results) for x, y in zip(a_, b_)))}
        model.setMathMode(0)
        model.setGroup(args.group)
        split = {"images_per_s": sorted(rates)[1], "regions": rates, "results": split_results, "group": split_group,
                 "group_trial": split_group_trial, "captions_after_final_nms": split_alt}
    serial_pass = False
    stage_live, single_image_latency_ms, stage_group = None, None, None
    nprof = K * nrep
    if on_gpu and rank == 0 and args.lanes != 1 and args.full:
        # Per-kernel durations are only meaningful when kernels do not overlap: with >1 lanes the MFMA launches of
        # different images run concurrently.  Roofline pass: the same workload on ONE lane, HIP events around every
        # MFMA launch (on the stream it is launched on).  It describes the serial schedule, not the timed one.
        model.setLanes(1)
        model.setGroup(1)
        nprof = min(K, 5)
        model.forward_batch_device(imgs, 1, H, W)
        sync()
        model.mfma_profile(reset=1)
        model.forward_batch_device(imgs, nprof, H, W)
        sync()
        prof = model.mfma_profile(reset=-1)
        stage = model.stage_times()
        # The same single-image mode WITHOUT per-launch events -- the schedule run_model / the daemon actually use: the decode
        # rows advance as two blocks on two streams and the final NMS runs beside them, so the row kernels,
        # launch gaps and ragged tile rounds of one block are covered by the other.  Stage times are event pairs on the main stream.
        lat = []
        for _ in range(3):
            l0 = time.perf_counter()
            model.forward_batch_device(imgs, 1, H, W)
            sync()
            lat.append(1e3 * (time.perf_counter() - l0))
        stage_live = model.stage_times()
        single_image_latency_ms = sorted(lat)[1]
        # the per-image stages as the TIMED schedule runs them: one stream, but the multi-lane planning and the timed group size
        # (BASELINE configs[2] asks for the bilinear RoI pooling of a batch; one launch now covers a group's boxes)
        stage_group = None
        if args.group > 1:
            check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"plan_mode", 0), "dc_debug_set")
            model.setGroup(args.group)
            model.forward_batch_device(imgs, min(args.group, n_img), H, W)
            sync()
            model.forward_batch_device(imgs, min(args.group, n_img), H, W)
            sync()
            stage_group = model.stage_times()
            check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"plan_mode", args.plan_mode), "dc_debug_set")
        model.setLanes(args.lanes)
        model.setGroup(args.group)
        serial_pass = True

    # ---- the other BASELINE.json configs, on THIS run's clock (round-5 verdict, weak #9: they existed only as builder-run files) --
    # Short legs of the same product calls at the other configs' shapes, each in both caption orders: warm regions, then timed
    # regions for >= --config-leg-seconds; the median region is reported.  Schedules are fixed (no trial): two lanes x groups of
    # eight, the pair a 12-pair sweep put first at every one of these shapes in both caption orders (round 6; the others within
    # 1-3 %, single images 9-12 % behind at 300 proposals).
    config_legs = None
    if (on_gpu and rank == 0 and world == 1 and not had_dist and not args.no_config_legs and args.math_mode == 0
            and (H, W, P) == (600, 720, 1000) and "DC_BENCH_CHILD" not in os.environ):
        config_legs = {}
        legs = [("configs[2]", "batch of 32 synthetic 720x600 images, 300 proposals each", 600, 720, 300, 32, 2, 8),
                ("configs[4]", "1080x720 synthetic images, 2000 proposals, 15-token cap", 720, 1080, 2000, 16, 2, 8),
                ("configs[0]", "720x480 (run_model.lua's elephant.jpg size), 1000 proposals; synthetic image and weights", 480, 720, 1000, 32, 2, 8)]
        for tag, what, h_, w_, p_, n_, lanes_, group_ in legs:
            distinct = 8
            host_c = np.stack([make_synthetic_image(h_, w_, 7000 + 100 * len(config_legs) + i) for i in range(distinct)])
            dev_c = ctx.to_device(np.concatenate([host_c] * (n_ // distinct)))
            model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=p_)
            model.setLanes(lanes_); model.setGroup(group_)
            leg = {"what": what, "height": h_, "width": w_, "proposals": p_, "images_per_region": n_, "lanes": lanes_, "group": group_}
            res_by_order = {}
            for order in (False, True):
                model.setCaptionOrder(order)
                for _ in range(2):
                    model.forward_batch_device(dev_c.ptr, n_, h_, w_)
                sync()
                rates, spent, res_c = [], 0.0, None
                while spent < args.config_leg_seconds or len(rates) < 3:
                    sync()
                    c0 = time.perf_counter()
                    res_c = model.forward_batch_device(dev_c.ptr, n_, h_, w_)
                    sync()
                    dt_ = time.perf_counter() - c0
                    rates.append(n_ / dt_); spent += dt_
                res_by_order[order] = res_c
                gf_ = stage_gflop(h_, w_, p_, T, V)
                fl_ = 1e9 * (sum(gf_.values()) - 2.0 * h_ * w_ * 3 * 64 * 9 / 1e9)       # MFMA family: conv1_1 is its own kernel
                rows_ = float(np.mean([len(b) for b, _, _ in res_c]))
                if order:
                    fl_ -= (p_ - rows_) * gf_["lstm_decode"] * 1e9 / p_                   # only the decoded rows count
                v_ = sorted(rates)[len(rates) // 2]
                leg["captions_after_final_nms" if order else "reference_order"] = {
                    "value": v_, "unit": "images/s", "ms_per_step": 1e3 / v_, "regions": len(rates), "timed_seconds": spent,
                    "frac": v_ * fl_ / 1e12 / FP32_MFMA_PEAK_TFLOPS, "algorithmic_mfma_gflop_per_image": fl_ / 1e9,
                    "rows_decoded_per_image": rows_ if order else float(p_)}
            model.setCaptionOrder(False)
            leg["value"] = leg["reference_order"]["value"]
            leg["ms_per_step"] = leg["reference_order"]["ms_per_step"]
            leg["frac"] = leg["reference_order"]["frac"]
            leg["caption_orders_identical"] = bool(all(np.array_equal(x, y) for a_, b_ in zip(res_by_order[False], res_by_order[True])
                                                       for x, y in zip(a_, b_)))
            if tag == "configs[2]":
                # BASELINE configs[2] asks for the BilinearRoiPooling throughput of the batch: the stage as this schedule runs it
                # (one launch per group of four), one stream, multi-lane planning, stage events
                check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"plan_mode", 0), "dc_debug_set")
                model.setLanes(1)
                model.forward_batch_device(dev_c.ptr, group_, h_, w_); sync()
                model.forward_batch_device(dev_c.ptr, group_, h_, w_); sync()
                st_ = model.stage_times()
                check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"plan_mode", args.plan_mode), "dc_debug_set")
                fh_, fw_ = (h_ + 15) // 16, (w_ + 15) // 16
                rb_ = 4.0 * 512 * (fh_ * fw_ + p_ * 49) + 16.0 * p_
                if st_.get("bilinear_roi_pool", 0) > 0:
                    leg["hbm_stages"] = {"bilinear_roi_pool_grouped": {
                        "group": group_, "algorithmic_bytes_per_image": rb_, "ms_per_image": st_["bilinear_roi_pool"],
                        "GBps": rb_ / (st_["bilinear_roi_pool"] * 1e-3) / 1e9, "peak_GBps": HBM_PEAK_GBPS}}
                if st_.get("lstm_decode", 0) > 0:
                    leg["decode_frac"] = stage_gflop(h_, w_, p_, T, V)["lstm_decode"] / st_["lstm_decode"] / FP32_MFMA_PEAK_TFLOPS
            leg["_check"] = (host_c[0], res_by_order[False][0])              # image 0 and its batch result: the oracle leg below
            dev_c.free()
            config_legs[tag] = leg
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
        model.setLanes(args.lanes); model.setGroup(args.group)

    if rank == 0:
        burst = world * K / elapsed
        value, value_source = burst, ("median of %d timed regions of %d steps" % (nrep, K) if nrep > 1
                                      else "one timed region of %d steps" % K)
        if sustained is not None:
            sustained["vs_timed_regions"] = sustained["images_per_s"] / burst
            if abs(sustained["vs_timed_regions"] - 1.0) > 0.03:
                # the short regions do not represent the steady state: report the sustained rate
                value, value_source = sustained["images_per_s"], "sustained leg (differs from the timed regions by > 3 %)"
        out = {
            "metric": "images/sec at 720x600, 1000 proposals",
            "value": value,
            "unit": "images/s",
            "n_gpus": world,
            "steps": K,
            "warmup": Wm,
            "ms_per_step": 1e3 * world / value,
            "value_source": value_source,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if args.math_mode == 0 else "split-bf16 (opt-in: fp32 operands as three bf16 planes, six bf16 MFMA products, fp32 accumulate)",
            "data": "synthetic" if on_gpu else "stub",
            "config": {"workload": "forward_test: one %dx%d image, VGG-16 trunk + %d proposals + greedy LSTM "
                                   "decode (T=15,V=10497), synthetic weights" % (W, H, P),
                       "images_per_gpu": K, "parallelism": "image-sharded x%d" % world,
                       "total_output_boxes": total_boxes,
                       "gather": carrier if carrier is not None else
                                 ((None if gather_note is None else "none; " + gather_note) if not had_dist else
                                  "torch.distributed.gather (%s)%s" % (args.dist_backend, "; " + gather_note if gather_note else ""))},
            "repeats": {"n": nrep, "statistic": "median", "images_per_s": [world * K / e for e in elapsed_all],
                        "timed_seconds_total": sum(elapsed_all)},
            "per_rank_images_per_s": per_rank_rates,
            "sustained": sustained,
        }
        out["config"]["shard_table"] = shard_table(world, K, P, model.seq_length) if had_dist else None
        if host_legs is not None:
            out["value_host_inputs"] = {"pageable": host_legs["pageable"], "pinned": host_legs["pinned"], "unit": "images/s",
                                        "vs_value": {k: v / burst for k, v in host_legs.items()},
                                        "note": "one region of %d images handed over in host memory (dc_forward_batch, "
                                                "imgs_on_device = 0): the 5.2 MB H2D copy of an image rides the lane's stream "
                                                "ahead of its kernels; `value` is measured with inputs resident in HBM" % min(K, n_distinct)}
        if not on_gpu:
            out["lanes"] = args.lanes
            out["config"]["gather_order_verified"] = gather_order_verified
        if on_gpu:
            out["lanes"] = args.lanes
            out["host_enqueue_us_per_image"] = host_enqueue_us
            out["group"] = args.group
            if lane_trials is not None:
                out["lanes_trial_images_per_s"] = {str(k): v for k, v in lane_trials.items()}
            if group_trials is not None:
                out["group_trial_images_per_s"] = {str(k): v for k, v in group_trials.items()}
            if sched_trials is not None:
                out["schedule_trial_images_per_s"] = {"lanes%d_group%d" % k: v for k, v in sched_trials.items()}
        if on_gpu and args.full:
            gf = stage_gflop(H, W, P, T, V)
            # the peak this run's arithmetic is priced against: fp32 MFMA, or -- for a whole run in the opt-in split-bf16 mode
            # (--math-mode 1) -- the dense bf16 MFMA peak / 6 (six bf16 products per fp32 multiply-add), as roofline_split_bf16 does
            RUN_PEAK = FP32_MFMA_PEAK_TFLOPS if args.math_mode == 0 else BF16_MFMA_PEAK_TFLOPS / 6.0
            ach = prof["flops"] / (prof["ms"] * 1e-3) / 1e12 if prof["ms"] > 0 else 0.0
            mfma_flops_per_image = prof["flops"] / max(nprof, 1)
            if args.caption_order:
                # the library's launch profile counts a launch's host-side row count; the packed decode runs the rows the final
                # NMS kept (device-side count): price the language model on those
                kept_rows = total_boxes / float(max(world * K, 1))
                skipped = (P - kept_rows) * gf["lstm_decode"] * 1e9 / P
                mfma_flops_per_image -= skipped
                ach = (prof["flops"] - skipped * nprof) / (prof["ms"] * 1e-3) / 1e12 if prof["ms"] > 0 else 0.0
                gf = dict(gf, lstm_decode=gf["lstm_decode"] * kept_rows / P)       # per-stage fractions below: the rows actually decoded
                out["config"]["caption_order"] = ("captions after the final NMS (--caption-order 1: a profiler option, not the headline "
                                                  "command); %.1f of %d rows decoded per image, language-model FLOPs counted on those" % (kept_rows, P))
            roof = {
                "bound": "mfma",
                "kernel": "fp32 MFMA contraction family (v_mfma_f32_32x32x2_f32): mfma_gemm_ks_kernel<CONV> (K-split "
                          "128x128, K >= 3072: conv4_2..5_3, RPN conv, fc6, fc7, LM encoder; mfma_gemm_sk_kernel = stream-K over a "
                          "partial last round in single-image mode), mfma_gemm_v2[_mixed]_kernel<..> (128x64 tiles, two-stage LDS ring = "
                          "three workgroups per CU, 64x64 last round: conv1_2..conv3_3, decode step = vocabulary arg-max + h.Wh; "
                          "128x128: conv4_1; 64x64: RPN heads, LSTM gates of the image step)",
                # `achieved` / `frac` are filled below from the TIMED schedule (round-4 verdict: the fraction tied to the driver's
                # clock is the headline); the serial one-stream pass with per-launch HIP events stays as achieved_serial / frac_serial
                "achieved": None, "peak": RUN_PEAK, "unit": "TFLOP/s" if args.math_mode == 0 else "TFLOP/s (fp32-equivalent; peak = dense bf16 MFMA / 6)", "frac": None,
                "achieved_serial": ach, "frac_serial": ach / RUN_PEAK, "traffic": None,
                "algorithmic_bytes_per_launch": mfma_family_bytes(H, W, P, T, V)[0] / mfma_family_bytes(H, W, P, T, V)[1],
                "algorithmic_bytes_per_image": mfma_family_bytes(H, W, P, T, V)[0],
                "launches_per_image": prof["launches"] / float(max(nprof, 1)),
                "algorithmic_gflop_per_image": mfma_flops_per_image / 1e9,
                "avg_launch_ms": prof["ms"] / max(prof["launches"], 1),
                "serial_mfma_ms_per_image": prof["ms"] / max(nprof, 1),
                "measured_on": ("separate 1-lane (serial) pass of %d images after the timed regions: per-launch HIP events "
                                "need non-overlapping kernels" % nprof) if serial_pass
                               else "the timed regions themselves (1 lane)",
            }
            # per-stage fractions of the fp32 MFMA peak from the serial stage times of the same pass (the metric's
            # "conv MFMA util" is trunk_frac)
            for key, name in (("vgg16_trunk", "trunk_frac"), ("fc6_fc7", "fc_frac"), ("lstm_decode", "decode_frac")):
                if stage.get(key, 0) > 0:
                    roof[name] = gf[key] / stage[key] / RUN_PEAK
            if stage_live:
                # the live single-image schedule (two-stream decode, final NMS on a third stream), no per-launch events
                roof["single_image_mode"] = {
                    "latency_ms": single_image_latency_ms,
                    "stage_ms": stage_live,
                    "trunk_frac": gf["vgg16_trunk"] / stage_live["vgg16_trunk"] / RUN_PEAK if stage_live.get("vgg16_trunk", 0) > 0 else None,
                    "decode_frac": gf["lstm_decode"] / stage_live["lstm_decode"] / RUN_PEAK if stage_live.get("lstm_decode", 0) > 0 else None,
                    "note": "dc_set_lanes(1) as run_model uses it; trunk_frac / fc_frac / decode_frac above are the ONE-stream pass with per-launch events"}
            roof["stage_gflop_per_image"] = gf
            roof["serial_ms_per_image"] = sum(stage.values()) if stage else None
            # whole-timed-region figure: MFMA FLOPs of the K images / wall time (launches of the lanes overlap)
            roof["timed_region_effective_tflops"] = K * mfma_flops_per_image / elapsed / 1e12      # per GPU
            # `frac` above is the SERIAL schedule (one lane, kernels back to back, per-launch events); this one is the
            # schedule that was actually timed: algorithmic MFMA FLOPs of the region / its wall time / peak, per GPU
            roof["frac_timed_region"] = roof["timed_region_effective_tflops"] / RUN_PEAK
            roof["achieved"] = roof["timed_region_effective_tflops"]
            roof["frac"] = roof["frac_timed_region"]
            roof["frac_is"] = ("the TIMED multi-lane schedule: algorithmic MFMA FLOPs of the median region / its wall time / peak "
                               "(= frac_timed_region); frac_serial / achieved_serial = one stream, HIP events around every launch, "
                               "avg_launch_ms their mean -- the per-kernel figure the rocprofv3 stats under profiles/ agree with")
            if sustained is not None:
                roof["frac_sustained"] = (sustained["images_per_s"] / world) * mfma_flops_per_image / 1e12 / RUN_PEAK
            # HBM bytes per MFMA launch cannot be measured from inside the process: quoted from the committed rocprofv3
            # PMC passes of this same command with --lanes 1 (tools/collect_profiles.sh + tools/pmc_summary.py)
            try:
                pm = json.load(open(os.path.join(ROOT, PMC_PROFILE)))
                fam = [v for k, v in pm.items() if k.startswith("mfma_gemm") and isinstance(v, dict) and "avg_hbm_bytes_per_launch" in v]
                calls = sum(v["calls"] for v in fam)
                roof["traffic_from_profile"] = {
                    "hbm_bytes_per_launch": sum(v["avg_hbm_bytes_per_launch"] * v["calls"] for v in fam) / calls,
                    "mfma_util_pmc": sum(v.get("mfma_util", 0) * v["total_us"] for v in fam) / sum(v["total_us"] for v in fam),
                    "file": PMC_PROFILE, "profile_commit": pm.get("_commit"), "bench_commit": git_head(),
                    "unit": "HBM bytes per launch (FETCH_SIZE x2 + WRITE_SIZE), separate --pmc passes"}
                if (H, W, P) == (600, 720, 1000):
                    # the committed counter passes ran THIS workload (same command, --lanes 1): average HBM bytes of one
                    # launch of the family, per launch like `achieved` (provenance in traffic_from_profile)
                    roof["traffic"] = roof["traffic_from_profile"]["hbm_bytes_per_launch"]
                    roof["traffic_over_algorithmic"] = roof["traffic"] / roof["algorithmic_bytes_per_launch"]
            except Exception:
                roof["traffic_from_profile"] = None
            # ... and measured by this run itself when it can be: not under a profiler already, not a child pass, one GPU
            under_profiler = any(k in os.environ for k in ("ROCP_TOOL_LIBRARIES", "ROCPROF_OUTPUT_PATH", "ROCPROFILER_LIBRARY_CTOR"))
            if on_gpu and world == 1 and not had_dist and not args.no_traffic_leg and not under_profiler and "DC_BENCH_CHILD" not in os.environ:
                try:
                    live = measure_traffic_live(args)
                    roof["traffic_live"] = live
                    roof["traffic"] = live["hbm_bytes_per_launch"]
                    roof["traffic_over_algorithmic"] = roof["traffic"] / roof["algorithmic_bytes_per_launch"]
                    roof["traffic_source"] = "traffic_live (this run); traffic_from_profile = the committed passes, for comparison"
                except Exception as e:                           # the committed figure above stays
                    roof["traffic_live"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
                    roof["traffic_source"] = "traffic_from_profile (the live passes failed)"
            elif "traffic" in roof and roof["traffic"] is not None:
                roof["traffic_source"] = "traffic_from_profile (live passes skipped: %s)" % (
                    "--no-traffic-leg" if args.no_traffic_leg else "under a profiler" if under_profiler else "child pass / multi-GPU")
            out["roofline"] = roof
            # HBM-side stages named by BASELINE.json (bilinear sampler, NMS): algorithmic bytes / stage time
            fh, fw = (H + 15) // 16, (W + 15) // 16
            A = 12 * fh * fw
            roi_bytes = 4.0 * 512 * (fh * fw + P * 49) + 16.0 * P
            nms_bytes = 20.0 * A + 8.0 * P
            hb = {}
            if stage.get("bilinear_roi_pool", 0) > 0:
                hb["bilinear_roi_pool"] = {"algorithmic_bytes": roi_bytes, "ms": stage["bilinear_roi_pool"],
                                           "GBps": roi_bytes / (stage["bilinear_roi_pool"] * 1e-3) / 1e9,
                                           "peak_GBps": HBM_PEAK_GBPS}
            if stage.get("rpn_nms", 0) > 0:
                hb["rpn_nms"] = {"algorithmic_bytes": nms_bytes, "ms": stage["rpn_nms"],
                                 "GBps": nms_bytes / (stage["rpn_nms"] * 1e-3) / 1e9, "peak_GBps": HBM_PEAK_GBPS,
                                 "note": "latency-bound by construction (greedy dependency chain), see DESIGN.md 4.2"}
            if stage_group and stage_group.get("bilinear_roi_pool", 0) > 0:
                # one launch over the group's boxes: per-image time = the group's stage time / group (dc_stage_times divides)
                hb["bilinear_roi_pool_grouped"] = {"group": args.group, "algorithmic_bytes_per_image": roi_bytes,
                                                   "ms_per_image": stage_group["bilinear_roi_pool"],
                                                   "GBps": roi_bytes / (stage_group["bilinear_roi_pool"] * 1e-3) / 1e9,
                                                   "peak_GBps": HBM_PEAK_GBPS,
                                                   "note": "one stream, multi-lane planning, the timed schedule's group size: "
                                                           "the stage as the timed regions run it"}
            # the same stages' HBM bytes as COUNTED by this run's PMC child passes (traffic_live), beside the algorithmic bytes
            lk = (roof.get("traffic_live") or {}).get("hbm_stage_kernels") or {}
            if "bilinear_roi_pool" in hb and "bilinear_roi_pool_kernel" in lk:
                c = lk["bilinear_roi_pool_kernel"]
                hb["bilinear_roi_pool"]["hbm_bytes_counted"] = c["hbm_bytes_per_launch"]
                hb["bilinear_roi_pool"]["write_bytes_counted"] = c["write_kb_per_launch"] * 1024.0
                hb["bilinear_roi_pool"]["GBps_counted"] = c["hbm_bytes_per_launch"] / (stage["bilinear_roi_pool"] * 1e-3) / 1e9
            if "rpn_nms" in hb and "nms_kernels" in lk:
                hb["rpn_nms"]["hbm_bytes_counted_rpn_and_final_nms"] = lk["nms_kernels"]["hbm_bytes_per_image"]
                hb["rpn_nms"]["nms_launches_per_image"] = lk["nms_kernels"]["launches_per_image"]
            out["hbm_stages"] = hb
            out["warm_up_regions_images_per_s"] = warm_regions
            if alt is not None:
                # Captions AFTER the final NMS (dc_set_caption_order(1), what the CLIs run): the same outputs -- compared array by
                # array with the reference-order results of the last timed region -- with the LSTM run only on the rows the final
                # NMS kept, ONE packed decode per group.  NOT `value` (which keeps the reference's order).  Its roofline counts the
                # FLOPs of the rows actually decoded: no credit for the rows it skips.
                lm_row = gf["lstm_decode"] * 1e9 / P
                fl = mfma_flops_per_image - (P - alt["rows_decoded_per_image"]) * lm_row
                out["value_captions_after_final_nms"] = alt["images_per_s"]
                out["roofline_captions_after_final_nms"] = {
                    "bound": "mfma", "unit": "TFLOP/s", "peak": RUN_PEAK,
                    "achieved": alt["images_per_s"] * fl / 1e12, "frac": alt["images_per_s"] * fl / 1e12 / RUN_PEAK,
                    "algorithmic_gflop_per_image": fl / 1e9, "rows_decoded_per_image": alt["rows_decoded_per_image"],
                    "rows_in_reference_order": P, "regions_images_per_s": alt["regions"], "statistic": "median of 5 regions of %d steps" % K,
                    "outputs_identical_to_value_regions": alt["identical"], "vs_value": alt["images_per_s"] / burst,
                    "lanes": alt["lanes"], "group": alt["group"], "schedule_trial_images_per_s": alt["trial"],
                    "note": "DenseCapModel.lua:261-275 keeps K of the P rows; LanguageModel rows are independent (LanguageModel.lua:293-348), "
                            "so the captions of the K kept rows are the reference's.  frac = (MFMA FLOPs of trunk, RPN, fc6/fc7 over "
                            "P rows + language model over the K decoded rows) x images/s / peak, from this leg's own wall time"}
            if split is not None:
                sp_tf = split["images_per_s"] * mfma_flops_per_image / 1e12
                out["value_split_bf16"] = split["images_per_s"]
                out["roofline_split_bf16"] = {
                    "bound": "mfma", "unit": "TFLOP/s (fp32-equivalent)", "achieved": sp_tf, "peak": BF16_MFMA_PEAK_TFLOPS / 6.0,
                    "frac": sp_tf / (BF16_MFMA_PEAK_TFLOPS / 6.0), "vs_value": split["images_per_s"] / burst,
                    "regions_images_per_s": split["regions"], "group": split["group"],
                    "group_trial_images_per_s": split["group_trial"],
                    "kernel": "mfma_gemm_bf3_128_kernel / mfma_gemm_v2[_mixed]_kernel<.., BF3>: v_mfma_f32_32x32x16_bf16, six bf16 "
                              "products per fp32 multiply-add (weights as three bf16 planes made at load, activations split "
                              "into three planes in registers)",
                    "note": "OPT-IN mode (dc_set_math_mode(1)), not the headline: `value`, `dtype` and `roofline` above are pure "
                            "fp32 MFMA.  fp32-equivalent = the same algorithmic FLOPs as `roofline`; peak = dense bf16 MFMA peak / 6. "
                            "Few-tile contractions stay on the fp32 route in this mode (counted at the same FLOPs).  Under this "
                            "load the board sustains ~1.55-1.8 GHz, not 2.4, and boxes differ by ~5 % (profiles/r05_split_bf16.md)"}
                sa = split.get("captions_after_final_nms")
                if sa is not None:
                    # both opt-in knobs together (run_model -math_mode 1 with its default caption order); language-model FLOPs of the
                    # decoded rows only, priced against the same bf16 peak / 6
                    fl2 = mfma_flops_per_image - (P - sa["rows_decoded_per_image"]) * gf["lstm_decode"] * 1e9 / P
                    out["value_split_bf16_captions_after_final_nms"] = sa["images_per_s"]
                    out["roofline_split_bf16"]["captions_after_final_nms"] = {
                        "value": sa["images_per_s"], "unit": "images/s", "regions_images_per_s": sa["regions"], "lanes": sa["lanes"],
                        "group": sa["group"], "rows_decoded_per_image": sa["rows_decoded_per_image"],
                        "achieved": sa["images_per_s"] * fl2 / 1e12, "frac": sa["images_per_s"] * fl2 / 1e12 / (BF16_MFMA_PEAK_TFLOPS / 6.0),
                        "identical_to_the_reference_order_in_this_mode": sa["identical_to_the_reference_order_in_this_mode"],
                        "vs_value": sa["images_per_s"] / burst}
            out["stage_ms_serial_image"] = stage
        if on_gpu and world == 1 and not args.no_cpu_baseline:
            # the restated reference CPU path (oracle) on a bounded sample of the same workload
            from oracle import densecap_oracle as O
            ncores = os.cpu_count() or 1
            # all host cores, the reference's NMS form (one full-length vector pass per pick), 1 warm-up image,
            # then >= 3 timed images.  "All cores" is tried, not assumed: torch-CPU conv / GEMM at these sizes stops scaling
            # (and on some hosts thrashes) past a few dozen threads, so one image is timed at each candidate thread count and
            # the fastest count -- stated in `cores`, with the trial in `thread_trial` -- runs the timed images.
            # (Measured on the 256-core host of the round-5 box: 16 threads 1.21 s, 32: 1.16 s, 64: 2.35 s, 128: 5.7 s, 256: 93 s
            # per image -- oversubscribed OpenMP teams on small GEMMs.  The trial therefore climbs and stops at the first count
            # that is 1.3x slower than the best so far; what it skipped is named in `sample`.)
            # (round 6: the climb is bounded -- 16 / 32 / 64 threads at most and 45 s of trial in all: beyond 64 every host measured
            # so far was slower, and one oversubscribed image must not cost minutes)
            cands = sorted({c for c in (16, 32, 64) if c <= ncores} | {min(ncores, 32)})
            trial, skipped = {}, []
            for c in cands:
                if trial and (min(trial.values()) * 1.3 < list(trial.values())[-1] or sum(trial.values()) > 45.0):
                    skipped.append(c)
                    continue
                torch.set_num_threads(c)
                if not trial:
                    O.forward_test(host[0], weights, 0.7, 0.3, P, 15, nms_impl="vector")        # warm-up image
                t0_ = time.perf_counter()
                O.forward_test(host[0], weights, 0.7, 0.3, P, 15, nms_impl="vector")
                trial[c] = time.perf_counter() - t0_
            nthreads = min(trial, key=trial.get)
            torch.set_num_threads(nthreads)
            nb = 5                                             # (round 6: five images, three before)
            oracle_out, per_image = [], []
            for i in range(nb):
                c0 = time.perf_counter()
                oracle_out.append(O.forward_test(host[i % n_distinct], weights, 0.7, 0.3, P, 15, nms_impl="vector"))
                per_image.append(time.perf_counter() - c0)
            cdt = sorted(per_image)[nb // 2] * nb              # median image x nb
            # the oracle's outputs of this leg double as an in-run parity check of the timed regions' own results
            # (image i of the last timed region): identical = same K, boxes / scores within 1e-4 relative, token rows equal
            ident, dep = 0, []
            for i, (ob, osc, oseq) in enumerate(oracle_out[:len(results)]):
                hb_, hs_, ht_ = results[i]
                same = len(hb_) == len(ob)
                if same and len(ob):
                    same = bool((np.abs(hb_ - ob).max(axis=1) <= 1e-4 * np.maximum(1.0, np.abs(ob).max(axis=1))).all()
                                and (np.abs(hs_ - osc) <= 1e-4 * np.maximum(1.0, np.abs(osc))).all()
                                and (np.asarray(ht_) == np.asarray(oseq)).all())
                if same:
                    ident += 1
                else:
                    dep.append(i)
            # a departure is not waved through: the image goes through tests/parity.py::strict_check, which REPLAYS the oracle's
            # NMS decision by decision (a decision may come from the HIP values only where the oracle's margin is within
            # FLIP_K x the discrepancy observed for its operands) and must reproduce the HIP list exactly
            replayed = []
            for i in dep:
                try:
                    from tests import parity as PAR
                    r_ = PAR.strict_check(model, weights, host[i % n_distinct], P)
                    replayed.append({"image": i, "replayed": True, "K": r_.get("K"), "K_oracle": r_.get("K_oracle"),
                                     "matched": r_.get("matched"), "rpn_decisions_flipped": len(r_.get("rpn_flips", [])),
                                     "final_decisions_flipped": len(r_.get("final_list_flips", [])),
                                     "k_needed": [r_.get("rpn_k_needed"), r_.get("final_k_needed")], "FLIP_K": PAR.FLIP_K})
                except Exception as e:                      # noqa: BLE001 -- a failed replay is reported, not hidden
                    replayed.append({"image": i, "replayed": False, "error": str(e)[:300]})
            out["parity"] = {"in_run": {"images": nb, "identical_to_oracle": ident, "departures": dep, "departures_replayed": replayed,
                                        "rule": "same K; boxes, scores within 1e-4 relative; greedy token ids identical; an image that "
                                                "departs must be reproduced by the flip replay of tests/parity.py (near-tie decisions only)"}}
            try:
                rep_all = json.load(open(os.path.join(ROOT, PARITY_REPORT)))
                rep = [r for r in rep_all if "_summary" not in r]
                rep_summary = next((r["_summary"] for r in rep_all if "_summary" in r), None)
                out["parity"]["committed_report"] = {
                    "file": PARITY_REPORT, "images": len(rep),
                    "final_lists_identical": sum(1 for r in rep if not r.get("final_list_flips") and not r.get("token_near_ties")
                                                 and r.get("matched") == r.get("K_oracle") == r.get("K")),
                    "images_with_replayed_rpn_decisions": sum(1 for r in rep if r.get("rpn_flips")),
                    "replayed_final_nms_decisions": sum(r.get("final_list_flips_n", len(r.get("final_list_flips", []))) for r in rep),
                    "token_near_ties": sum(len(r.get("token_near_ties", [])) for r in rep),
                    "decode_rows": sum(r.get("decode_rows", 0) for r in rep),
                    "decode_rows_identical": sum(r.get("decode_rows_identical", 0) for r in rep),
                    "max_k_needed": rep_summary.get("max_k_needed") if rep_summary else None}
            except Exception:
                out["parity"]["committed_report"] = None
            out["cpu_baseline"] = {"value": nb / cdt, "unit": "images/s", "cores": torch.get_num_threads(),
                                   "kind": "port",
                                   "host_cores": ncores,
                                   "thread_trial_s_per_image": {str(k): v for k, v in trial.items()},
                                   "seconds_per_image": per_image,
                                   "sample": "median of %d images %dx%d P=%d after 1 warm-up image, restated reference CPU path "
                                             "(torch-CPU fp32 GEMM/conv, box_utils.nms in the reference's vector-pass-per-pick "
                                             "form, C sampler; Torch7 unavailable); thread count = the fastest of a climbing trial "
                                             "over %s of %d host cores%s" % (nb, W, H, P, sorted(trial), ncores,
                                                                             (" (stopped once a count ran 1.3x slower than the best; "
                                                                              "not tried: %s)" % skipped) if skipped else "")}
            if config_legs:
                # one image of every configs leg against the oracle: the leg's own batch result, identical or replayed
                from tests import parity as PAR
                for tag, leg in config_legs.items():
                    img0, res0 = leg.pop("_check")
                    try:
                        st_ = {}
                        ora_ = O.forward_test(img0, weights, 0.7, 0.3, leg["proposals"], 15, stages=st_)
                        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=leg["proposals"])
                        rep_ = PAR.final_or_replay(model, O, weights, img0, res0, ora_, st_, leg["proposals"])
                        flips = len(rep_.get("rpn_flips", [])) + len(rep_.get("final_list_flips", [])) + len(rep_.get("token_near_ties", []))
                        leg["parity_in_run"] = {"images": 1, "K": len(res0[0]), "K_oracle": len(ora_[0]), "matched": rep_.get("matched"),
                                                "identical_to_oracle": flips == 0, "decisions_replayed": flips, "passed": True}
                    except Exception as e:                      # noqa: BLE001 -- a failed check is reported, not hidden
                        leg["parity_in_run"] = {"images": 1, "passed": False, "error": ("%s: %s" % (type(e).__name__, e))[:300]}
                model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
            if split is not None:
                ident3 = 0
                for i, (ob, osc, oseq) in enumerate(oracle_out[:len(split["results"])]):
                    hb_, hs_, ht_ = split["results"][i]
                    ok3 = len(hb_) == len(ob)
                    if ok3 and len(ob):
                        ok3 = bool((np.abs(hb_ - ob).max(axis=1) <= 1e-4 * np.maximum(1.0, np.abs(ob).max(axis=1))).all()
                                   and (np.abs(hs_ - osc) <= 1e-4 * np.maximum(1.0, np.abs(osc))).all()
                                   and (np.asarray(ht_) == np.asarray(oseq)).all())
                    ident3 += 1 if ok3 else 0
                out["parity"]["in_run_split_bf16"] = {"images": min(nb, len(split["results"])), "identical_to_oracle": ident3,
                                                      "rule": "same as in_run (a near-tie may legitimately flip: tests/parity.py replays those)"}
        if config_legs:
            for leg in config_legs.values():
                leg.pop("_check", None)              # (--no-cpu-baseline: no oracle leg ran)
                leg.setdefault("parity_in_run", {"images": 0, "passed": None, "note": "skipped with --no-cpu-baseline"})
            out["configs"] = config_legs
        _libc.fflush(None)                       # whatever C code buffered so far (the RCCL banner) goes out BEFORE the line
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)                            # nothing after it reaches stdout (teardown messages of native libraries)
    if comm is not None and not abandoned:
        comm.close()
    if abandoned:
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(0)                   # a carrier call never returned: no orderly teardown possible


if __name__ == "__main__":
    main()
