#!/usr/bin/env python3
"""bench.py — MultiCol-SLAM feature front end + brute-force matcher on MI355X.

A "step" = one pass of the hot path over one batch of synthetic input already resident in HBM: F multi-frames per GPU -> extraction (pyramid, FAST,
oct-tree, orientation, blur, descriptors + masks, rays) -> brute-force Hamming matching.  value = features extracted AND matched per second, whole job.

Workloads (one engine, `Job`; --workload):
  stream  (default)  BASELINE configs[1], the configuration the metric is quoted on: 3-camera 754x480 multi-frames, mdBRIEF, N = 1000, every
                     multi-frame matched with SearchByBoW(KF,KF) (masked Hamming, ratio 0.9) against the multi-frame before it.
  db                 BASELINE configs[2]: the same stream, every multi-frame against 32 stored multi-keyframes (SearchByBoW(KF,F) with the vocabulary
                     restriction removed; the relocalisation loop src/cTracking.cpp:1125-1221) — the matcher dominates.
  rig / rig8         BASELINE configs[3] / [4]: 6-camera (8-camera) 1280x800 rig, 2000 features per camera, against 32 (256) stored keyframes.
  --mode orb --nfeatures 400 on any of them = the reference's shipped extractor settings (Examples/Lafida/Slam_Settings_indoor1.yaml:12-39).

N > 1 (one process per GPU, torch.distributed backend nccl = RCCL): BASELINE north_star's split, see multicol-slam_amd/rig.py — the (camera, frame)
images of a step are sharded camera-major over the ranks, ONE all-gather of descriptor|mask|count blocks per step, the gathered buffer is consumed in
place, the (frame, keyframe) pairs are sharded.  Per-GPU work is fixed (F multi-frames and F x keyframes pairs per GPU): weak scaling.  N = 1 runs the
same code without the collective.  Barrier + max-over-ranks timing.

A plain run (`python bench.py --gpus 1 --steps N --warmup W`) sets up, warms up, times the N steps, writes the last timed step's outputs if --dump-outputs
DIR is given, and prints the result line.  Everything else needs --full: the oracle check of the timed output, the roofline block (per-kernel passes of its
own), and for the default workload the further legs below and the CPU baseline.

Legs of a --full run besides the headline (each checked against the oracle): `e2e` — the same step with host buffers at the boundary (images up through the SDMA
engine on a stream picked by the library's hardware-queue probe, results down through mcs_copy_narrow on the context's result stream; --e2e-sweep "h2d:d2h,..."
and the MCS_E2E_* variables are its A/B switches, tools/ab_e2e.sh) —, configs[2] at 16 multi-frames per step with its own e2e leg, the reference's
shipped ORB settings, the N > 1 exchange path at world size 1 over RCCL, and last the CPU baseline.  Every leg runs `settle_steps` untimed steps in front of its
warm-up (GPU clocks), reported in the line.  `python bench.py --gpus N` outside a launcher starts its N ranks itself.

torch is plumbing only (device memory, stream handle, process group); all compute is libmcs_hip.so through its C ABI.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# HIP streams share a small pool of hardware queues (4 by default), and streams on one queue run in order: with the context's three streams, torch's and RCCL's
# the exchange kernels of the N > 1 step landed on the main stream's queue and stalled it (2.28 -> 2.16 ms per step with 8 queues, measured at world size 1 with
# --exchange nccl1).  Only for the multi-process runs: which streams share a queue is the runtime's choice, and in the N = 1 default run — more streams: the e2e
# leg's two copy streams — 8 queues measured WORSE for the e2e leg (3.2 against 2.4 ms) and for the exchange_world1 leg (2.9 against 2.35); the headline is 2.08 ms
# either way.  Read by the HIP runtime at its first call; a host application sets it the same way.
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
# multi-process GPU work on these hosts needs dmabuf IPC (without it RCCL fails with hipIpcGetMemHandle: invalid argument); exported on the boxes, kept here for a bare environment
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# the oracle (checks, CPU baseline) is OpenMP code: its idle worker threads must not spin on the CPUs the host thread enqueues from (libgomp reads this when it loads)
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np  # noqa: E402

MODES = {"orb": (0, 0), "dbrief": (1, 0), "mdbrief": (1, 1)}
KERNELS = ("pyramid", "fast", "octree", "blur", "describe", "describe_fast", "match", "greedy")
E2E_H2D, E2E_D2H = "runtime", "2"   # how the e2e leg moves its page-locked buffers unless MCS_E2E_H2D / MCS_E2E_D2H say otherwise (run_e2e): the runtime's SDMA copy in, mcs_copy_narrow with TWO workgroups out (they saturate the link's write direction; more of them stall every other kernel's memory traffic)
TIE_SLOTS = 256   # entries per capture slot of the in-loop tie enforcement (the default band lists about one keypoint per 64-multi-frame step)
POOL = 64   # distinct synthetic multi-frames the stream cycles through: 8 scenes of 8 frames each ((3,1)-px shifts), synth.stream_image
WORKLOADS = {
    #          ncam  W     H    nfeat  F/GPU  keyframes  name in BASELINE.json
    "stream": (3, 754, 480, 1000, 64, 0, "configs[1]"),
    "db": (3, 754, 480, 1000, 64, 32, "configs[2]"),
    "rig": (6, 1280, 800, 2000, 4, 32, "configs[3]"),
    "rig8": (8, 1280, 800, 2000, 1, 256, "configs[4]"),
}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="stream", choices=list(WORKLOADS))
    ap.add_argument("--frames", type=int, default=0, help="multi-frames per step and GPU (default: per workload)")
    ap.add_argument("--mode", default="mdbrief", choices=list(MODES))
    ap.add_argument("--nfeatures", type=int, default=0, help="features per camera (default: per workload)")
    ap.add_argument("--ncam", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--keyframes", type=int, default=-1, help="stored keyframes every multi-frame is matched against (0 = the multi-frame before it)")
    ap.add_argument("--topk", type=int, default=32)
    ap.add_argument("--full", action="store_true", help="besides the headline: the oracle check of the timed output, the roofline block (per-kernel passes of "
                                                        "their own) and, for the default workload, the e2e / configs[2] / shipped-settings / latency / batch-sweep / "
                                                        "RCCL world-1 legs and the CPU baseline")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps write what the last timed step handed its caller as DIR/<name>.npy "
                                                                      "(float32 / float64, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="(--full) skip the e2e / configs[2] / shipped-settings legs of the default run")
    ap.add_argument("--cpu-frames", type=int, default=0, help="multi-frames in the bounded CPU-baseline sample (default: 3 x cpu quota, >= 48)")
    ap.add_argument("--check", action="store_true", help="verify the timed output against the oracle (implied by --full)")
    ap.add_argument("--no-check", action="store_true", help="skip the oracle check of the timed output, also under --full (profiling runs)")
    ap.add_argument("--e2e-sweep", default="", help="A/B of the e2e leg's copy mechanism: comma list of H2D:D2H settings, each 'runtime' or a workgroup count "
                                                    "(e.g. runtime:runtime,16:16,16:runtime); runs only the headline job and those e2e legs")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: build the multi-GPU plan (slabs, exchange runs, pair ownership, buffer sizes) of every workload for "
                                                          "--gpus N (N = 1: for 2, 4 and 8) and check it; non-zero exit on the first violated property")
    ap.add_argument("--exchange", default="auto", choices=["auto", "nccl1"],
                    help="nccl1: run the N > 1 code path (separate send buffers, asynchronous all_gather_into_tensor on RCCL, work.wait(), three buffer sets, "
                         "matching one step late) at world size 1 over the nccl backend")
    return ap.parse_args(argv)


def free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def launch_ranks(args):
    """`python bench.py --gpus N` outside a launcher: start the N ranks here (one process per GPU, torch.distributed.run on 127.0.0.1 with a free port) and hand
    back their exit code; rank 0 of the children prints the JSON line on our stdout.  The reference's own split is one worker per camera of a multi-frame
    (`#pragma omp parallel for num_threads(nrCams)`, /root/reference/src/cMultiFrame.cpp:128-164); here one process per GPU."""
    import subprocess
    if os.environ.get("MCS_BENCH_SHARE_GPU") != "1":    # before any rank starts: N ranks need N GPUs (the ranks check again, each for itself)
        import torch
        if torch.cuda.device_count() < args.gpus:
            raise SystemExit("bench.py: --gpus %d but only %d GPU(s) visible (MCS_BENCH_SHARE_GPU=1 runs the ranks on one GPU over gloo: a functional run, not a "
                             "measurement)" % (args.gpus, torch.cuda.device_count()))
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "8")            # see the note at the top of this file: the exchange needs hardware queues of its own
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    env["MCS_BENCH_LAUNCHED"] = "1"
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def dry_run(args):
    """The plan of every workload at the world sizes the driver's SCALE run uses, checked without a GPU (multicol-slam_amd/rig.py plan_check): what the first
    multi-GPU execution relies on is index arithmetic, and a wrong plan must fail HERE, loudly, not as a silent wrong buffer on eight GPUs."""
    rig = importlib.import_module("multicol-slam_amd.rig")
    worlds = [args.gpus] if args.gpus > 1 else [2, 4, 8]
    report, failed = [], False
    for name, (ncam, W, H, nfeat, F, D, cfg) in WORKLOADS.items():
        if args.workload != "stream" and name != args.workload:
            continue
        F, D = args.frames or F, (D if args.keyframes < 0 else args.keyframes)
        cap = (args.nfeatures or nfeat) + 3 * 8   # keypoint rows per image of the usual configurations (nfeatures + 3 per level, 8 levels)
        for world in worlds:
            row = {"workload": name, "config": cfg, "world": world}
            try:
                row.update(rig.plan_check(args.ncam or ncam, F, world, cap, D, 32, args.topk))
                row["plan_digest"] = rig.plan_digest(args.ncam or ncam, F, world, cap, D, 32, args.topk).hex()   # what every rank of the real run prints and compares
                row["image_bytes_per_rank"] = row["images_per_rank"] * W * H
                row["ok"] = True
            except ValueError as ex:
                row["ok"], row["error"] = False, str(ex)
                failed = True
            report.append(row)
    print(json.dumps({"dry_run": report, "ok": not failed}))
    return 1 if failed else 0


_WATCHDOGS = []


def watchdog(seconds, what):
    """A hang in the first multi-rank RCCL calls (rendezvous, the first collective) must end loudly: after `seconds` the rank prints its distributed / RCCL environment
    and leaves with exit code 3.  Returns a function that retires the watchdog."""
    import threading

    def fire():
        keys = ["RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY", "GPU_MAX_HW_QUEUES", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES",
                "NCCL_DEBUG", "NCCL_SOCKET_IFNAME", "NCCL_P2P_DISABLE", "NCCL_SHM_DISABLE", "NCCL_IB_DISABLE", "RCCL_MSCCL_ENABLE", "TORCH_NCCL_ASYNC_ERROR_HANDLING", "MCS_BENCH_SHARE_GPU"]
        sys.stderr.write("bench.py: WATCHDOG — %s did not finish within %d s on rank %s; environment:\n%s\n"
                         % (what, seconds, os.environ.get("RANK", "0"), "\n".join("  %s=%s" % (k, os.environ.get(k, "(unset)")) for k in keys)))
        sys.stderr.flush()
        os._exit(3)
    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    _WATCHDOGS.append(t)
    return t.cancel


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


class Env:
    pass


def torch_empty_like_cpu(t):
    import torch
    return torch.empty(t.shape, dtype=t.dtype)


def setup(args):
    import torch
    import torch.distributed as dist
    e = Env()
    e.torch, e.dist = torch, dist
    e.rank = int(os.environ.get("RANK", "0"))
    e.world = int(os.environ.get("WORLD_SIZE", "1"))
    e.local = int(os.environ.get("LOCAL_RANK", "0"))
    # MCS_BENCH_SHARE_GPU=1: functional test of the N>1 code path on a 1-GPU box (all ranks on cuda:0, gloo for the collectives)
    e.share = os.environ.get("MCS_BENCH_SHARE_GPU") == "1"
    if e.share:
        e.local = 0
    # refuse to lie: the line's n_gpus is the number of ranks that ran, and it must be what --gpus asked for, each rank on a GPU of its own
    if e.world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE is %d (launch with --nproc-per-node %d, or let bench.py start the ranks itself)" % (args.gpus, e.world, args.gpus))
    if not e.share and torch.cuda.device_count() < max(args.gpus, 1):
        raise SystemExit("bench.py: --gpus %d but only %d GPU(s) visible (MCS_BENCH_SHARE_GPU=1 runs the ranks on one GPU over gloo: a functional run, not a measurement)"
                         % (args.gpus, torch.cuda.device_count()))
    e.backend = None
    e.exchange = e.world > 1          # the step runs the exchange (send buffer -> all-gather -> late matching); world 1 normally has nothing to exchange
    if e.world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        e.backend = "gloo" if e.share else "nccl"
        done = watchdog(int(os.environ.get("MCS_BENCH_INIT_TIMEOUT", "420")), "the rendezvous + first barrier (init_process_group, %s)" % e.backend)   # ranks of a fresh box import torch for up to two minutes each
        dist.init_process_group(e.backend, rank=e.rank, world_size=e.world)
        if e.backend == "nccl":
            torch.cuda.set_device(e.local)
            dist.barrier(device_ids=[e.local])   # the communicator is created HERE (lazily, by the first collective), not in the first timed step
        else:
            dist.barrier()
        done()
    torch.cuda.set_device(e.local)
    e.dev = torch.device("cuda", e.local)
    e.red_dev = torch.device("cpu") if e.share else e.dev
    e.mcs = importlib.import_module("multicol-slam_amd")
    e.synth = importlib.import_module("multicol-slam_amd.synth")
    e.rig = importlib.import_module("multicol-slam_amd.rig")
    e.lib = e.mcs.lib()
    # one explicit (non-default) stream shared by torch's copies, the collective's hand-over and the library's kernels: their order is the enqueue order
    e.stream = torch.cuda.Stream(device=e.dev)
    torch.cuda.set_stream(e.stream)
    assert e.stream.cuda_stream != 0
    e.ctx = e.mcs.Context(e.local, e.stream.cuda_stream)
    e.async_collectives = None        # probed by the first exchange
    return e


def force_exchange_world1(e):
    """--exchange nccl1: a one-rank RCCL process group, and the step takes the N > 1 code path"""
    if e.world != 1:
        raise SystemExit("--exchange nccl1 is a world-size-1 run")
    if not e.dist.is_initialized():
        import socket
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            sk.close()
        done = watchdog(int(os.environ.get("MCS_BENCH_INIT_TIMEOUT", "420")), "the one-rank RCCL group (init_process_group + first barrier)")
        e.dist.init_process_group("nccl", rank=0, world_size=1)
        e.dist.barrier(device_ids=[e.local])   # the communicator is created HERE (lazily, by the first collective: tens of seconds on a fresh box), not under the 60-s watchdog of the first exchange
        done()
    e.backend = "nccl"
    e.exchange = True


def sync_all(e):
    e.torch.cuda.synchronize(e.dev)
    if e.world > 1:
        e.dist.barrier()
    e.torch.cuda.synchronize(e.dev)


SETTLE = int(os.environ.get("MCS_BENCH_SETTLE", "32"))   # untimed steps in FRONT of the W warm-up steps of every leg: the GPU's clocks need ~50 ms of work to come up from
                                                         # idle (the first twenty steps behind an idle stretch run 2-3 % slow: 1.575 against 1.55 ms); reported as "settle_steps"


def timed(e, step, warmup, steps, status):
    for _ in range(SETTLE):
        step()
    for _ in range(warmup):
        step()
    sync_all(e)
    status()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync_all(e)
    el = time.perf_counter() - t0
    status()
    return el


def kernel_times(e, step, reps=5):
    """per-kernel time of one step from the library's HIP events on its own stream (side-stream overlap off while timing, so each kernel is measured alone)"""
    e.ctx.enable_timing(True)
    acc = {}
    for _ in range(reps):
        step()
        e.torch.cuda.synchronize(e.dev)
        for name in KERNELS:
            try:
                acc[name] = acc.get(name, 0.0) + e.ctx.kernel_ms(name)
            except e.mcs.McsError:
                pass
    e.ctx.enable_timing(False)
    return {k: v / reps for k, v in acc.items()}


def pmc_entry_parts(tag, names):
    """HBM bytes (FETCH_SIZE + WRITE_SIZE) per launch of the named kernels from the committed counter passes, or None"""
    try:
        ks = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["workloads"][tag]["kernels"]
        parts = [ks[n] for n in names if n in ks]
        return int(sum(k["fetch_kib"] + k["write_kib"] for k in parts) * 1024) if parts else None
    except (OSError, KeyError, ValueError, TypeError):
        return None


def pmc_entry(tag, dom):
    """HBM bytes (FETCH_SIZE + WRITE_SIZE) and VALU wave-instructions per launch of kernel `dom` from the committed counter passes of this workload"""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        ks = t["workloads"][tag]["kernels"]
        # "keypoints" = the keypoint stage: oct-tree + orientation (its tail), keypoint records / rays, descriptors
        doms = ("octree", "orient_a", "orient_b", "describe", "describe_list", "describe_exact") if dom == "keypoints" else ("match", "match_expand") if dom == "match" else (dom,)
        parts = [ks[n] for n in doms if n in ks]
        if not parts:
            return None, None
        return int(sum(k["fetch_kib"] + k["write_kib"] for k in parts) * 1024), sum(k.get("valu_insts", 0) for k in parts)
    except (OSError, KeyError, ValueError, TypeError):
        return None, None


# ------------------------------------------------------------------------------------------------ the job
class Spec:
    def __init__(self, args, world):
        ncam, W, H, nfeat, F, D, cfg = WORKLOADS[args.workload]
        self.name, self.cfg = args.workload, cfg
        self.ncam = args.ncam or ncam
        self.W, self.H = args.width or W, args.height or H
        self.nfeat = args.nfeatures or nfeat
        self.F = args.frames or F
        self.D = D if args.keyframes < 0 else args.keyframes
        self.mode, self.topk = args.mode, args.topk
        self.world = world
        self.tag = "%s-%s-%dx%dx%d-n%d-f%d-k%d" % (self.name, self.mode, self.ncam, self.W, self.H, self.nfeat, self.F, self.D)


_IMAGE_CACHE = {}


class Job:
    """One rank's share of a workload: its slab of (camera, frame) images, the exchange, its share of the (frame, keyframe) pairs."""

    def __init__(self, e, sp, n_image_buffers=1, n_sets=0):
        torch, mcs, synth, rig = e.torch, e.mcs, e.synth, e.rig
        self.e, self.sp = e, sp
        dev = e.dev
        do_db, masks_on = MODES[sp.mode]
        self.masks_on = masks_on
        base_cams = synth.lafida_cameras()
        self.cams = [base_cams[c % 3] if (sp.W, sp.H) == (754, 480) else synth.scaled_camera(base_cams[c % 3], sp.W, sp.H) for c in range(sp.ncam)]
        FT = sp.F * e.world
        # a first, tiny extractor only to learn the row capacity; the real one is sized for the slab
        probe = mcs.Extractor(e.ctx, sp.W, sp.H, max_batch=1, nfeatures=sp.nfeat, do_dBrief=do_db, learnMasks=masks_on)
        cap = probe.cap
        self.level_sizes = probe.level_sizes
        probe.close()
        self.lay = lay = rig.RigLayout(sp.ncam, FT, e.world, cap, 32)
        self.L, self.cap, self.FT = lay.L, cap, FT
        # what a rank holds after the exchange: the whole [camera][frame] array (all-gather: the database sweeps need every multi-frame), or — when every
        # multi-frame only meets its predecessor — just its own frames and one predecessor, sent point to point (rig.RingExchange)
        self.ring = rig.RingExchange(lay) if (e.exchange and sp.D == 0 and os.environ.get("MCS_BENCH_RING_ALLGATHER") != "1") else None
        self.view = self.ring.view if self.ring else lay
        self.ex = mcs.Extractor(e.ctx, sp.W, sp.H, max_batch=lay.L, nfeatures=sp.nfeat, do_dBrief=do_db, learnMasks=masks_on)
        slab = lay.slab(e.rank)
        self.slab = slab
        # synthetic inputs of this rank's slab (untimed).  Global frame f shows synthetic frame f % POOL: every rank carries the same amount of work
        def image(c, f):   # the legs of one bench run share their synthetic images
            key = (sp.W, sp.H, c, f % POOL)
            if key not in _IMAGE_CACHE:
                _IMAGE_CACHE[key] = synth.stream_image(f, c, self.cams[c], POOL)
            return _IMAGE_CACHE[key]
        self.imgs_np = np.stack([image(c, f) for c, f in slab])
        mm = [synth.mirror_mask(cam) for cam in self.cams]
        self.masks_np = np.stack([mm[c] for c, _ in slab])
        self.d_imgs = [torch.from_numpy(self.imgs_np).to(dev) for _ in range(n_image_buffers)]
        self.d_masks = torch.from_numpy(self.masks_np).to(dev)
        self.camarr = (mcs.Ocam * lay.L)(*[mcs.make_ocam(self.cams[c]) for c, _ in slab])
        # Buffer sets in rotation.  Every leg runs the same pipelined order (round 6): a call extracts set n, then — on the host — waits for the capture event of
        # set n - 1 only, recomputes that batch's rounding-tie keypoints with the host's libm and patches its device rows (mcs_extractor_patch_ties), and only
        # then enqueues the exchange and the (deferred) search of set n - 1, which run beside the extraction of set n.  Three sets: being extracted, being
        # exchanged / matched, still read by the search issued one call earlier.
        self.nsets = n_sets or 3
        self.xs = torch.cuda.Stream(device=dev) if e.exchange and e.backend == "nccl" else None   # where collectives are issued from (exchange_begin)
        self.sets = [self._make_set() for _ in range(self.nsets)]
        self.cur = 0
        # before the first exchange: every rank prints the digest of the plan it computed from its own arguments (the bytes `--dry-run` prints) and the ranks
        # compare — an all-gather of 32 bytes; a rank that diverges is named and the run aborts before any buffer is exchanged
        self.plan_digest = None
        if e.exchange:
            dg = rig.plan_digest(sp.ncam, sp.F, e.world, cap, sp.D, 32, sp.topk)

            def gather32(b):
                t = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(e.red_dev)
                out_t = torch.empty(32 * e.world, dtype=torch.uint8, device=e.red_dev)
                e.dist.all_gather_into_tensor(out_t, t)
                return out_t.cpu().numpy().tobytes()
            print("bench.py: rank %d of %d plan digest %s (%s)" % (e.rank, e.world, dg.hex(), sp.tag), file=sys.stderr)
            done = watchdog(int(os.environ.get("MCS_BENCH_EXCHANGE_TIMEOUT", "60")), "the plan-digest all-gather (32 bytes)")
            try:
                self.plan_digest = rig.check_plan_digests(dg, e.rank, e.world, gather32)
            except ValueError as ex:
                raise SystemExit("bench.py: %s" % ex)
            done()
        # stored keyframes of this rank (database sweeps): contiguous sets of ncam*cap rows, filled once from an untimed pass
        self.kfs = lay.keyframe_shard(sp.D, e.rank) if sp.D > 0 else []
        self.nkf = len(self.kfs)
        if sp.D > 0:
            nk = max(self.nkf, 1)
            self.db = torch.zeros((nk, lay.rows_frame, lay.row_stride), dtype=torch.uint8, device=dev)
            self.db_valid = torch.zeros((nk, lay.rows_frame), dtype=torch.uint8, device=dev)
            self._fill_database()
        self.matched_set = self.sets[0]
        # deferred searches: lists + greedy pass of step n run on the library's own stream beside the extraction of step n + 1; the fence before a buffer
        # set is reused gives back the ordering a single stream would have had (include/mcs_c.h: mcs_ctx_set_async_search)
        self.async_search = os.environ.get("MCS_BENCH_ASYNC_SEARCH", "1") != "0"
        mcs.check(e.lib.mcs_ctx_set_async_search(e.ctx.h, 1 if self.async_search else 0))
        # rounding ties are enforced INSIDE the loop: a capture slot per buffer set; MCS_BENCH_TIE_BAND widens the band (tests: 2e-4 px lists every fallback)
        self.ties_in_loop = os.environ.get("MCS_BENCH_TIES_IN_LOOP", "1") != "0"
        self.ties_listed = self.ties_patched = 0
        if os.environ.get("MCS_BENCH_TIE_BAND"):
            self.ex.set_tie_band(float(os.environ["MCS_BENCH_TIE_BAND"]))
        if self.ties_in_loop:
            self.ex.set_tie_capture(self.nsets, TIE_SLOTS)
        # prime the pipeline: the first step() patches, exchanges and matches the multi-frames extracted here
        self.extract(self.sets[self.nsets - 1])
        if e.exchange:
            done = watchdog(int(os.environ.get("MCS_BENCH_EXCHANGE_TIMEOUT", "60")), "the first descriptor exchange (%s)" % ("point-to-point ring" if self.ring else "all-gather"))
            try:
                self.step()
                torch.cuda.synchronize(dev)
                done()
            except (RuntimeError, TypeError, ValueError) as ex:
                if self.ring is None:
                    raise
                # a torch / RCCL build without grouped point-to-point operations (the failure is the same on every rank): the frame ring falls back to the
                # all-gather, which delivers a superset of what the ring exchange would; said in the output (config.parallelism names the form used)
                print("bench.py: ring exchange unavailable (%s: %s), using the all-gather" % (type(ex).__name__, str(ex)[:200]), file=sys.stderr)
                self.ring, self.view = None, lay
                torch.cuda.synchronize(dev)
                self.sets = [self._make_set() for _ in range(self.nsets)]
                self.matched_set = self.sets[0]
                self.cur = 0
                self.extract(self.sets[self.nsets - 1])
                self.step()
                torch.cuda.synchronize(dev)
                done()

    def _make_set(self):
        torch, lay, dev, e = self.e.torch, self.lay, self.e.dev, self.e
        b = Env()
        view = self.view
        b.G = torch.zeros(view.images_total * lay.block_bytes, dtype=torch.uint8, device=dev)         # gathered [camera][frame][cap+1][64] (ring exchange: F + 1 local frames)
        b.send = torch.zeros(lay.send_bytes, dtype=torch.uint8, device=dev) if e.exchange else b.G   # no exchange: the slab IS the whole array
        b.valid = torch.zeros(view.images_total * lay.rows_img, dtype=torch.uint8, device=dev)
        b.nkp = torch.zeros(lay.L, dtype=torch.int32, device=dev)
        if self.xs is not None:
            b.ev_done, b.ev_x = torch.cuda.Event(), torch.cuda.Event()
        b.nkp_all = torch.zeros(view.images_total, dtype=torch.int32, device=dev)
        b.kps = torch.zeros((lay.L * self.cap, 7), dtype=torch.float32, device=dev)
        b.rays = torch.zeros((lay.L * self.cap, 3), dtype=torch.float64, device=dev)
        if self.sp.D > 0:
            nk = max(len(lay.keyframe_shard(self.sp.D, e.rank)), 1)
            b.match = torch.full((self.FT * nk * lay.rows_frame,), -1, dtype=torch.int32, device=dev)
            b.nmatch = torch.zeros(self.FT * nk, dtype=torch.int32, device=dev)
            b.fb = torch.zeros(self.FT * nk, dtype=torch.int32, device=dev)
        else:
            b.match = torch.full((self.sp.F * lay.rows_frame,), -1, dtype=torch.int32, device=dev)
            b.nmatch = torch.zeros(self.sp.F, dtype=torch.int32, device=dev)
            b.fb = torch.zeros(self.sp.F, dtype=torch.int32, device=dev)
        return b

    def frame_set(self, b, frame=0):
        """mcs_desc_set of multi-frame `frame` inside the gathered array of buffer set b"""
        mcs, lay = self.e.mcs, self.view
        doff, moff, voff, n, stride, brows, bpitch, _ = lay.frame_desc_set(frame)
        g, v = b.G.data_ptr(), b.valid.data_ptr()
        return mcs.DescSet(g + doff, (g + moff) if self.masks_on else None, v + voff, None, n, stride, brows, bpitch)

    def extract(self, b, img_buf=0):
        e, lay, lib, mcs, W, H = self.e, self.lay, self.e.lib, self.e.mcs, self.sp.W, self.sp.H
        sp_ = b.send.data_ptr()
        self.ex.extract_strided(lay.L, self.d_imgs[img_buf].data_ptr(), W * H, W, self.d_masks.data_ptr(), W * H, W, self.camarr, b.nkp.data_ptr(),
                                b.kps.data_ptr(), sp_, sp_ + lay.desc_size, b.rays.data_ptr(), lay.rows_img, lay.row_stride)
        mcs.check(lib.mcs_rig_pack_headers(e.ctx.h, C.c_void_p(b.nkp.data_ptr()), lay.L, self.cap, C.c_void_p(sp_), lay.row_stride))
        if self.xs is not None:
            b.ev_done.record(e.stream)

    def exchange_begin(self, b):
        """the one exchange step: descriptor | mask | count blocks of every rank's slab.  RCCL: asynchronous, and issued from a side stream that waits for THIS
        set's extraction only: torch orders a collective behind everything on the stream it is issued from, and in the pipelined step order the extraction of the
        next slab is already enqueued on the main stream — issued from there the exchange would start when that extraction ends and sit on the critical path."""
        e = self.e
        if not e.exchange:
            return None
        if self.xs is not None:
            self.xs.wait_event(b.ev_done)
            with e.torch.cuda.stream(self.xs):
                w = self._exchange_begin(b)
                b.ev_x.record(self.xs)
            return w
        return self._exchange_begin(b)

    def _exchange_begin(self, b):
        e = self.e
        if self.ring is not None:   # point to point: only the blocks this rank's pairs read
            if e.backend == "nccl":   # at world size 1 the rank's own blocks go through RCCL as well (a self send / receive), so that the path runs there
                return e.rig.ring_exchange_begin(self.ring, e.rank, b.send, b.G, self_via_p2p=e.world == 1)
            send_h, recv_h = b.send.cpu(), torch_empty_like_cpu(b.G)   # gloo: functional runs on one shared GPU bounce through host memory
            e.rig.ring_exchange_end(e.rig.ring_exchange_begin(self.ring, e.rank, send_h, recv_h))
            b.G.copy_(recv_h)
            return None
        if e.backend == "nccl":
            if e.async_collectives is None:   # probed once: a torch without the async_op keyword takes the blocking form (no overlap, same result);
                try:                          # any other failure of the collective propagates
                    w = e.dist.all_gather_into_tensor(b.G, b.send, async_op=True)
                    e.async_collectives = True
                    return w
                except TypeError:
                    e.async_collectives = False
            if e.async_collectives:
                return e.dist.all_gather_into_tensor(b.G, b.send, async_op=True)
            e.dist.all_gather_into_tensor(b.G, b.send)
            return None
        b.G.copy_(e.rig.all_gather_blocks(b.send, e.world))   # gloo: functional runs on one shared GPU
        return None

    def exchange_end(self, b, work):
        e, lay, lib, mcs = self.e, self.lay, self.e.lib, self.e.mcs
        if isinstance(work, list):
            e.rig.ring_exchange_end(work)
        elif work is not None:
            work.wait()                                        # a stream-side wait: later work on our stream is ordered behind the collective
        if self.xs is not None:
            e.stream.wait_event(b.ev_x)                        # (and behind the local copies of the ring exchange, made on the side stream)
        mcs.check(lib.mcs_rig_rows_valid(e.ctx.h, C.c_void_p(b.G.data_ptr()), self.view.images_total, self.cap, lay.row_stride, C.c_void_p(b.valid.data_ptr()),
                                         C.c_void_p(b.nkp_all.data_ptr())))

    def extract_and_exchange(self, b, img_buf=0):
        self.extract(b, img_buf)
        self.exchange_end(b, self.exchange_begin(b))

    def _fill_database(self):
        """untimed: the stored keyframes are earlier multi-frames of the same synthetic stream (keyframe k = multi-frame k % frames_total of one pass)"""
        torch, lay = self.e.torch, self.lay
        b = self.sets[0]
        self.extract(b)
        torch.cuda.synchronize(self.e.dev)
        self.ex.fix_ties()               # the stored keyframes' rows are the host libm's too (synchronous form: this pass is untimed)
        self.exchange_end(b, self.exchange_begin(b))
        torch.cuda.synchronize(self.e.dev)
        rows = b.G.view(lay.images_total, lay.rows_img, lay.row_stride)
        val = b.valid.view(lay.images_total, lay.rows_img)
        for j, k in enumerate(self.kfs):
            f = k % self.FT
            for c in range(lay.ncam):
                x = lay.image_index(c, f)
                self.db[j, c * self.cap:(c + 1) * self.cap] = rows[x, :self.cap]
                self.db_valid[j, c * self.cap:(c + 1) * self.cap] = val[x, :self.cap]
        torch.cuda.synchronize(self.e.dev)

    def match(self, b):
        e, lay, lib, mcs, sp = self.e, self.lay, self.e.lib, self.e.mcs, self.sp
        fr = self.frame_set(b, 0)
        if sp.D == 0:   # every multi-frame of this rank's range against the one before it (a ring over the step's frames; local array: frames 1 .. F)
            nft, first = (sp.F + 1, 1) if self.ring else (self.FT, e.rank * sp.F)
            mcs.check(lib.mcs_search_kf_kf_ring(e.ctx.h, nft, first, sp.F, C.byref(fr), lay.rows_img, 32, 0.9, sp.topk, mcs.MEM_DEVICE,
                                                C.c_void_p(b.match.data_ptr()), C.c_void_p(b.nmatch.data_ptr()), C.c_void_p(b.fb.data_ptr())))
        elif self.nkf:  # every multi-frame of the step against every stored keyframe of this rank
            d = self.db.data_ptr()
            kf = mcs.DescSet(d, (d + lay.desc_size) if self.masks_on else None, self.db_valid.data_ptr(), None, lay.rows_frame, lay.row_stride)
            mcs.check(lib.mcs_search_kf_f_sweep(e.ctx.h, self.nkf, C.byref(kf), lay.rows_frame, self.FT, C.byref(fr), lay.rows_img, 32, 0.9, sp.topk,
                                                mcs.MEM_DEVICE, C.c_void_p(b.match.data_ptr()), C.c_void_p(b.nmatch.data_ptr()), C.c_void_p(b.fb.data_ptr())))

    def patch(self, back=1):
        """the rounding-tie keypoints of the batch extracted `back` calls ago: recomputed on the host, the device rows patched (waits for that batch only)"""
        if self.ties_in_loop:
            listed, fixed = self.ex.patch_ties(back)
            self.ties_listed += listed
            self.ties_patched += fixed

    def step(self, img_buf=0):
        """One step = one extraction, one exchange, one matching pass per call, pipelined: enqueue the extraction of this step's slab; wait (host) for the
        PREVIOUS step's capture event and patch its rounding-tie rows; start that slab's exchange (N > 1; issued from the side stream, so the collective runs
        beside this step's kernels: the main stream meets it only AFTER this step's extraction, when it has long finished) and, stream-ordered behind it, match
        those multi-frames on the deferred streams.  The device never waits for the host: when the previous extraction ends,
        this one is already queued.  Results one step late."""
        b = self.sets[self.cur]
        p = self.sets[(self.cur - 1) % self.nsets]   # the set extracted in the previous call
        self.cur = (self.cur + 1) % self.nsets
        # the search that last read b is the one issued before the latest (the matcher of call n - 2 read the set extracted in call n - 3)
        self.e.mcs.check(self.e.lib.mcs_ctx_search_fence(self.e.ctx.h, 1))
        self.extract(b, img_buf)
        self.patch(1)
        self.exchange_end(p, self.exchange_begin(p))
        self.match(p)
        self.matched_set = p
        return b

    def last(self):
        """the buffer set whose matching pass was issued last"""
        return self.matched_set

    def status(self):
        self.ex.status()

    # ---- accounting
    def local_features(self):
        return int(self.last().nkp.sum().item())

    def pairs_per_step_local(self):
        b = self.last()
        if self.ring:
            nk = b.nkp_all.view(self.lay.ncam, self.sp.F + 1).sum(0).to(self.e.torch.float64)
            return float((nk[1:] * nk[:-1]).sum().item())
        nk = b.nkp_all.view(self.lay.ncam, self.FT).sum(0).to(self.e.torch.float64)   # features per multi-frame
        if self.sp.D == 0:
            fr = [f for f, _ in self.lay.frame_pairs(self.e.rank)]
            pr = [p for _, p in self.lay.frame_pairs(self.e.rank)]
            return float((nk[fr] * nk[pr]).sum().item())
        return float(self.db_valid.sum().item()) * float(nk.sum().item()) if self.nkf else 0.0

    def close(self):
        self.ex.close()


def roofline_block(sp, job, kern, feats_local, pairs_local):
    """`roofline` of the dominant KERNEL of one step on this rank — a single launch, named as the profile names it: algorithmic bytes per launch (SURVEY.md §8d /
    DESIGN.md §4) over its measured duration.  The keypoint STAGE it belongs to (oct-tree + orientation + records + descriptors) is a sub-key."""
    nimg = job.L
    md = sp.mode == "mdbrief"
    per_kp = 845 + 512 * (3 if md else 1) + 28 + 32 + (32 if md else 0)
    S = [w * h for w, h in job.level_sizes]
    rows = job.lay.rows_frame
    nsets = sp.F if sp.D == 0 else job.nkf * job.FT
    width = 64 if job.masks_on else 32
    kern = dict(kern)
    mfma = "match" in kern and job.lay.desc_size in (16, 32) and not os.environ.get("MCS_MATCH_VALU")   # launch_match(): no count_le, no camera groups here
    # one entry per KERNEL (pyramid: the seven k_resize_cols launches of the chain, summed): algorithmic bytes per launch.  The descriptor kernel's bytes are the
    # pattern samples + keypoint record + descriptor (+ mask): the 845-byte orientation disc is read by k_octree's tail, where it is counted.
    alg = {"describe_fast": (per_kp - 845) * feats_local, "octree": 845 * feats_local, "pyramid": nimg * (sum(S) - S[-1] + sum(S) - S[0]),
           "fast": nimg * sum(S), "blur": nimg * 2 * sum(S),
           # matcher: every set pair reads its query and train rows once (descriptor + mask) and writes K list entries per query row
           "match": (nsets * 2 * rows * width + nsets * rows * 4 * sp.topk) if "match" in kern else 0}
    # (octree: the orientation discs of the selected keys; the candidate lists it selects from are written and read inside the stage, not algorithmic input)
    names = {"describe_fast": "k_describe" if sp.mode == "orb" else "k_describe_fast", "octree": "k_octree", "pyramid": "k_resize_cols (x%d)" % (len(S) - 1), "fast": "k_fast_cells",
             "blur": "k_blur", "match": "k_match_mfma" if mfma else "k_match_partial"}
    pmc_name = {"describe_fast": ("describe_exact",) if sp.mode == "orb" else ("describe",), "octree": ("octree",), "pyramid": ("pyramid",), "fast": ("fast",), "blur": ("blur",), "match": ("match",)}
    governing = {"describe_fast": "latency of a wave's dependent chains (LDS gathers of the camera table + cross-lane sums) at 4 waves per SIMD; VALU and LDS each ~0.6-0.7 busy",
                 "octree": "latency (a chain of passes per workgroup; L1 line fills of the orientation tail)", "pyramid": "launch / memory latency of the small levels",
                 "fast": "VALU issue", "blur": "memory pipeline (load-8 / store-4 per lane)", "match": "matrix-core operand chain + VALU append (waits 45 % of wave cycles)"}
    single = [k for k in alg if k in kern and k != "pyramid" and kern[k] > 0]
    dom = max(single, key=lambda k: kern[k])
    ach = alg[dom] / (kern[dom] * 1e-3) / 1e9
    traffic = pmc_entry_parts(sp.tag, pmc_name[dom])
    _, valu = pmc_entry(sp.tag, pmc_name[dom][0])
    out = {"kernel": names[dom], "bound": "hbm", "achieved": round(ach, 2), "peak": 8000.0, "unit": "GB/s",
           "frac": round(ach / 8000.0, 5), "traffic": traffic, "alg_bytes_per_launch": int(alg[dom]), "avg_launch_ms": round(kern[dom], 4),
           "governing_bound": governing[dom],
           "per_kernel_ms": {k: round(v, 4) for k, v in kern.items()},
           "per_kernel_alg_GBps": {names[k]: round(alg[k] / (kern[k] * 1e-3) / 1e9, 1) for k in alg if k in kern and kern[k] > 0},
           "traffic_source": "profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command on the builder's GPU box, committed; fetch = 2 x FETCH_SIZE: "
                             "every read request of this chip's L2 is 128 bytes and is tallied as 64, profiles/r06/pmc_calibration.txt; Infinity-Cache hits are counted)" if traffic else None,
           "traffic_measured_in_this_run": False,
           "traffic_over_algorithmic": round(traffic / alg[dom], 3) if traffic and alg[dom] else None,
           "note": "`bound` / `peak` price the kernel against HBM because BASELINE.json asks for that fraction; no kernel of this path is HBM-bound — `governing_bound` names what "
                   "limits this one, `valu_issue` and (matcher) the matrix-core fraction carry the numbers: DESIGN.md §6"}
    flop_pair = 2 * 8 * job.lay.desc_size * (2 if job.masks_on else 1)   # a pair distance = one dot product over K = 8 * bytes (x2 with masks), DESIGN.md §4c
    if dom == "match" and mfma:   # the dominant kernel runs on the matrix cores: price it against the dense FP4 MFMA peak
        tf = pairs_local * flop_pair / (kern[dom] * 1e-3) / 1e12
        out.update({"bound": "mfma", "achieved": round(tf, 1), "peak": 10000.0, "unit": "TFLOP/s", "frac": round(tf / 10000.0, 4),
                    "alg_flop_per_launch": int(pairs_local * flop_pair), "hbm_alg_GBps": round(ach, 2)})
    if valu:
        peak = 1024 * 2.4e9 / 4 / 1e9
        a = valu / (kern[dom] * 1e-3) / 1e9
        out["valu_issue"] = {"wave_insts_per_launch": int(valu), "achieved": round(a, 1), "peak": round(peak, 1), "unit": "G wave-instructions/s", "frac": round(a / peak, 3)}
    if "octree" in kern and "describe" in kern:
        # the keypoint STAGE as one unit on SURVEY §8d's per-keypoint bytes (orientation disc 845 B + pattern samples + keypoint + descriptor [+ mask]): k_octree
        # (selection + orientation of the selected keys in its tail), k_orient_b (records, rays), the descriptor kernels
        st_ms, st_b = kern["octree"] + kern["describe"], per_kp * feats_local
        st_tr, st_valu = pmc_entry(sp.tag, "keypoints")
        out["stage"] = {"name": "keypoint stage: k_octree + " + ("k_describe" if sp.mode == "orb" else "k_orient_b + k_describe_fast + k_describe_list"), "alg_bytes_per_step": int(st_b),
                        "ms": round(st_ms, 4), "achieved_GBps": round(st_b / (st_ms * 1e-3) / 1e9, 2), "frac": round(st_b / (st_ms * 1e-3) / 1e9 / 8000.0, 5), "traffic": st_tr,
                        "traffic_over_algorithmic": round(st_tr / st_b, 3) if st_tr and st_b else None}
    if "match" in kern and pairs_local > 0:
        # 2 x 8 bit-ops (2.4 cycles) + 2 x 8 bit-counts (4.3 cycles) per 64 masked pairs and SIMD (tools/valu_latency.hip): the arithmetic alone
        cyc = (16 * 2.4 + 16 * 4.3) if job.masks_on else (8 * 2.4 + 8 * 4.3)
        ceiling = 1024 * 2.4e9 / cyc * 64
        pps = pairs_local / (kern["match"] * 1e-3)
        out["matcher"] = {"kernel": "k_match_mfma" if mfma else "k_match_partial", "pair_distances_per_launch": pairs_local, "Tpairs_per_s": round(pps / 1e12, 3),
                          "valu_kernel_ceiling_Tpairs_per_s": round(ceiling / 1e12, 3), "vs_valu_kernel_ceiling": round(pps / ceiling, 3)}
        if mfma:
            out["matcher"].update({"mfma_ceiling_Tpairs_per_s": round(1e16 / flop_pair / 1e12, 2), "mfma_frac": round(pps * flop_pair / 1e16, 4)})
    return out


DUMP_BYTES = 60 * 10 ** 6   # --dump-outputs: the most a dump may write (under 64 MB with the .npy headers)


def dump_outputs(e, job, d):
    """--dump-outputs DIR: what the last timed step handed its caller — the buffer set whose search that step issued (Job.step: results one step late) — as
    DIR/<name>.npy: per image the keypoint count, and over the valid rows the keypoint records (x, y, size, angle, response, octave, class_id), rays,
    descriptors and (mdBRIEF) masks as the search read them, then the search's match indices and per-pair match counts.  Descriptor and mask bytes are
    stored as little-endian 16-bit words, every integer exactly in float32; rays float64; matches one row per (frame, keyframe) pair.  Over DUMP_BYTES in all,
    every array of 1 MiB or more keeps the same fraction of its rows, drawn with a fixed seed (the drawn row numbers in <name>_rows.npy)."""
    lay, view = job.lay, job.view
    b = job.last()
    e.torch.cuda.synchronize(e.dev)
    nkp = b.nkp.cpu().numpy().astype(np.int64)
    own = np.concatenate([i * job.cap + np.arange(n) for i, n in enumerate(nkp)])   # rows of this rank's images that hold a keypoint
    kp = b.kps.cpu().numpy().view(np.uint8).reshape(-1, 28)[own].copy().view(e.mcs.KP_DTYPE).reshape(-1)
    valid = b.valid.cpu().numpy().reshape(-1) != 0
    rows = b.G.cpu().numpy().reshape(view.images_total * lay.rows_img, lay.row_stride)[valid]
    ds = lay.desc_size
    out = {"keypoint_counts": nkp.astype(np.float32),
           "keypoints": np.stack([kp[f].astype(np.float32) for f in kp.dtype.names], axis=1),
           "rays": b.rays.cpu().numpy()[own],
           "descriptors": np.ascontiguousarray(rows[:, :ds]).view("<u2").astype(np.float32)}
    if job.masks_on:
        out["masks"] = np.ascontiguousarray(rows[:, ds:2 * ds]).view("<u2").astype(np.float32)
    match = b.match.cpu().numpy()
    out["matches"] = match.astype(np.float32 if np.abs(match).max(initial=0) < (1 << 24) else np.float64).reshape(-1, lay.rows_frame)
    out["match_counts"] = b.nmatch.cpu().numpy().astype(np.float32)
    if sum(a.nbytes for a in out.values()) > DUMP_BYTES:
        big = [name for name in out if out[name].nbytes >= 1 << 20]
        room = DUMP_BYTES - sum(a.nbytes for name, a in out.items() if name not in big) - 8 * sum(len(out[name]) for name in big)   # less the row numbers (float64)
        keep = room / sum(out[name].nbytes for name in big)
        rng = np.random.default_rng(0)
        for name in big:
            n = len(out[name])
            r = np.sort(rng.choice(n, max(1, int(n * keep)), replace=False))
            out[name], out[name + "_rows"] = out[name][r], r.astype(np.float64)
    os.makedirs(d, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(d, name + ".npy"), a)


def run_job(e, sp, args, steps, warmup, want_roofline=True, check=True, dump=None):
    job = Job(e, sp)
    elapsed = timed(e, job.step, warmup, steps, job.status)
    if dump and e.rank == 0:
        dump_outputs(e, job, dump)
    x0 = job.ex.describe_stats()[0]
    job.step()
    exact_kp = job.ex.describe_stats()[0] - x0   # keypoints the guarded fast descriptor pass handed to the exact pass in one (untimed) step
    tie = job.ex.tie_stats()                     # the run's closest approach of an exact-arithmetic cvRound argument to a rounding tie (pixels)
    # ties are ENFORCED inside the loop (round 6): every step patched the previous step's listed rows on the host before that set's exchange and search were
    # enqueued (Job.step), so every row any timed search consumed is the host libm's — listed == patched over all steps is the statement
    tie_listed, _, tie_band = job.ex.tie_counts()
    feats_local = job.local_features()
    pairs_local = job.pairs_per_step_local()
    b = job.last()
    matches = int(b.nmatch.sum().item())
    rescans = int(b.fb.sum().item())
    elapsed_max, feats_all = e.rig.reduce_timing(elapsed, feats_local, e.red_dev, e.world)
    _, pairs_all = e.rig.reduce_timing(elapsed, pairs_local, e.red_dev, e.world)
    elapsed_min = -e.rig.reduce_timing(-elapsed, 0, e.red_dev, e.world)[0]   # the fastest rank (max of the negated times)
    checked = check_against_oracle(e, sp, job) if (check and e.rank == 0) else None   # before the per-kernel passes: the output of the timed configuration
    if check and e.rank == 0 and not e.exchange and sp.D == 0:
        # host copies of the set the loop matched last: main() compares ALL multi-frames and pairs of the CPU-baseline sample with it (check_full)
        lb = job.last()
        job.snapshot = {k: getattr(lb, k).cpu().numpy() for k in ("G", "kps", "match", "nmatch")}
    kern = kernel_times(e, job.step) if want_roofline else None   # every rank: step() contains the collective
    roof = roofline_block(sp, job, kern, feats_local, pairs_local) if (want_roofline and e.rank == 0) else None
    value = feats_all * steps / elapsed_max / 1e6
    what = ("cORBmatcher BF-Hamming SearchByBoW(KF,KF) vs the multi-frame before it" if sp.D == 0 else
            "cORBmatcher BF-Hamming SearchByBoW(KF,F) (vocabulary restriction removed) vs %d stored keyframes" % sp.D)
    cfg = {"workload": "BASELINE %s: %d-camera %dx%d multi-frames, %s extract (N=%d, 8 levels, FAST 20) + %s; %d multi-frames (%d images) per step per GPU, "
                       "inputs resident in HBM" % (sp.cfg, sp.ncam, sp.W, sp.H, sp.mode, sp.nfeat, what, sp.F, sp.F * sp.ncam),
           "multi_frames_per_step_per_gpu": sp.F, "distinct_multi_frames_in_the_stream": POOL, "features_per_step": int(feats_all),
           "pair_distances_per_step": pairs_all, "Gpairs_per_s": round(pairs_all * steps / elapsed_max / 1e9, 1),
           "matches_per_step_rank0": matches, "greedy_rescans_rank0": rescans, "topk": sp.topk, "stored_keyframes": sp.D,
           "descriptor_exact_pass_keypoints_per_step_rank0": exact_kp,
           # device libm vs the reference's can only round a coordinate differently within ~1e-13 px of a tie: this run's margin, measured over every cvRound
           # argument of the exact arithmetic (all warm-up and timed steps); null if no exact-arithmetic coordinate occurred
           "min_distance_to_a_rounding_tie_px_rank0": (tie if tie != float("inf") else None),
           "rounding_tie_band_px": tie_band, "keypoints_listed_within_the_band_all_steps_rank0": int(tie_listed),
           "ties_patched_in_loop": bool(job.ties_in_loop), "ties_listed_at_patch_time_rank0": int(job.ties_listed), "ties_recomputed_on_the_host_in_loop_rank0": int(job.ties_patched),
           "n_ranks": e.world, "collective_backend": e.backend, "tag": sp.tag, "plan_digest_all_ranks_agree": job.plan_digest,
           "ms_per_step_slowest_rank": round(elapsed_max / steps * 1e3, 4), "ms_per_step_fastest_rank": round(elapsed_min / steps * 1e3, 4),
           "exchange_bytes_received_per_rank_per_step": (0 if not e.exchange else job.ring.bytes_received(e.rank) if job.ring else job.lay.send_bytes * (e.world - 1)),
           "ranks_share_one_gpu": bool(e.share),
           "parallelism": ("single GPU, no collective" if not e.exchange else
                           ("camera-major image slabs x%d + 1 point-to-point exchange per step of the camera blocks of this rank's frames and one predecessor "
                            "(%d KiB received per rank; the all-gather would deliver %d KiB) + frame pairs sharded x%d"
                            % (e.world, job.ring.bytes_received(e.rank) // 1024, job.lay.send_bytes * (e.world - 1) // 1024, e.world)) if job.ring else
                           "camera-major image slabs x%d + 1 all-gather of descriptor blocks per step (%d KiB per rank, %s) + (frame, keyframe) pairs sharded x%d"
                           % (e.world, job.lay.send_bytes // 1024, "asynchronous, finished one step later" if e.async_collectives else "blocking", e.world))}
    if checked is not None:
        cfg["oracle_checked"] = job.checked
    out = {"metric": "Mfeatures/s extract+match, %d-cam %dx%d multi-frame" % (sp.ncam, sp.W, sp.H), "value": round(value, 3), "unit": "Mfeatures/s",
           "n_gpus": e.world, "steps": steps, "warmup": warmup, "settle_steps": SETTLE, "ms_per_step": round(elapsed_max / steps * 1e3, 4), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "u8+i32 (images, Hamming) / f64 (omni model)", "data": "synthetic", "config": cfg, "roofline": roof}
    if checked is not None:
        out["oracle_check"] = checked
    return job, out


# ------------------------------------------------------------------------------------------------ end-to-end (host buffers in and out)
def run_e2e(e, sp, steps, warmup, check=True):
    """The same step with the boundary's host buffers: images start in page-locked host memory (three device buffers in turn, hipMemcpyAsync = the SDMA engine, on a copy
    stream), keypoints, descriptor | mask blocks, counts and match arrays end in page-locked host memory (mcs_copy_narrow, two workgroups, on the context's result
    stream right behind the search that completes them), both overlapped with the compute of the neighbouring steps.  N = 1 only."""
    torch = e.torch
    NI = int(os.environ.get("MCS_E2E_IMAGE_BUFFERS", "3"))   # image buffers on the device: the upload runs up to two steps ahead
    job = Job(e, sp, n_image_buffers=NI, n_sets=3)
    NS = job.nsets
    upload_conflicts = None
    if os.environ.get("MCS_E2E_STREAMS", "probed").startswith("prio:"):   # A/B: explicit priorities (-1 high, 0 normal, 1 low), e.g. prio:0:1
        hip = C.CDLL("libamdhip64.so")
        hs = []
        for pr in os.environ["MCS_E2E_STREAMS"].split(":")[1:3]:
            h = C.c_void_p()
            assert hip.hipStreamCreateWithPriority(C.byref(h), 1, int(pr)) == 0
            hs.append(h)
        cin, cout = (torch.cuda.ExternalStream(h.value, device=e.dev) for h in hs)
    elif os.environ.get("MCS_E2E_STREAMS", "probed") == "probed":   # the upload stream the library picked by probing the hardware queues (mcs_ctx_transfer_stream)
        h, m = C.c_void_p(), C.c_uint()
        e.mcs.check(e.lib.mcs_ctx_transfer_stream(e.ctx.h, C.byref(h), C.byref(m)))
        upload_conflicts = m.value
        cin, cout = torch.cuda.ExternalStream(h.value, device=e.dev), torch.cuda.Stream(device=e.dev)
    elif os.environ.get("MCS_E2E_STREAMS", "plain") == "null":   # the uploads on the device's null stream (no new stream, no new pairing with a hardware queue)
        cin, cout = torch.cuda.default_stream(e.dev), torch.cuda.Stream(device=e.dev)
    else:                                                   # two plain streams (cout only serves MCS_E2E_OUT=stream)
        cin, cout = torch.cuda.Stream(device=e.dev), torch.cuda.Stream(device=e.dev)
    if os.environ.get("MCS_E2E_DIAG"):
        m = C.c_uint()
        e.mcs.check(e.lib.mcs_ctx_stream_conflicts(e.ctx.h, cin.cuda_stream, C.byref(m)))
        sys.stderr.write("e2e diag: upload stream shares a hardware queue with context streams (bit 0 main, 1 side, 2 matcher, 3 greedy): 0x%x\n" % m.value)
    h_img = [torch.from_numpy(job.imgs_np.copy()).pin_memory() for _ in range(NI)]
    outs = []
    for b in job.sets:
        outs.append([(t, torch.empty(t.shape, dtype=t.dtype).pin_memory()) for t in (b.send, b.nkp, b.kps, b.match, b.nmatch)])
    ev_in = [torch.cuda.Event() for _ in range(NI)]
    ev_free = [torch.cuda.Event() for _ in range(NI)]     # compute no longer reads image buffer i
    ev_done = [torch.cuda.Event() for _ in range(NS)]     # outputs of buffer set k complete
    ev_out = [torch.cuda.Event() for _ in range(NS)]      # outputs of buffer set k copied out
    state = {"i": 0, "worst": [0.0] * 4}

    # How the page-locked buffers travel: the runtime's own copy (torch copy_ -> hipMemcpyAsync: host -> device goes through the SDMA engine and occupies no CU;
    # device -> host runs as chip-wide blit kernels beside the step's kernels) or the library's narrow copy kernel (mcs_copy_narrow: a few workgroups).  Measured
    # (profiles/r04): H2D runtime + D2H narrow is the fast pairing; a narrow kernel reading host memory is the slow one.  MCS_E2E_H2D / MCS_E2E_D2H = "runtime" | "<workgroups>"
    wg_in, wg_out = (0 if v == "runtime" else -1 if v == "off" else int(v) for v in (os.environ.get("MCS_E2E_H2D", E2E_H2D), os.environ.get("MCS_E2E_D2H", E2E_D2H)))

    def travel(dst, src, wg, stream):
        if wg < 0:      # "off": A/B of the leg's event structure without the copy (run with --no-check)
            return
        if wg > 0:
            e.mcs.check(e.lib.mcs_copy_narrow(e.ctx.h, dst.data_ptr(), src.data_ptr(), dst.numel() * dst.element_size(), wg, stream.cuda_stream))
        else:
            dst.copy_(src, non_blocking=True)

    def upload(i):   # images of buffer i: page-locked host memory -> device, on the copy stream, once the kernels no longer read the buffer
        with torch.cuda.stream(cin):
            cin.wait_event(ev_free[i])
            travel(job.d_imgs[i], h_img[i], wg_in, cin)
            ev_in[i].record(cin)

    # Results leave on the RESULT stream (mcs_ctx_result_stream: the greedy pass's), right behind the search that completes them — no event in front, no further
    # stream.  (Round 3's form — a copy stream of its own, ordered by an event, two steps late — went with the pipelined order of round 6.)
    h = C.c_void_p()
    e.mcs.check(e.lib.mcs_ctx_result_stream(e.ctx.h, C.byref(h)))
    rstream = torch.cuda.ExternalStream(h.value, device=e.dev)

    def download_behind_search(k):
        with torch.cuda.stream(rstream):
            for src, dst in outs[k]:
                travel(dst, src, wg_out, rstream)
            ev_out[k].record(rstream)

    # The host stays at most AHEAD steps in front of the GPU (it waits for the results of step n - AHEAD to have reached host memory — which a live caller does
    # anyway, it consumes them): run far ahead, the runtime's H2D copy call blocks the host for 7-14 ms at a time every few dozen steps and the GPU runs dry behind it
    AHEAD = int(os.environ.get("MCS_E2E_AHEAD", "3"))

    MARK = int(os.environ.get("MCS_E2E_MARK", "1"))
    marks = [torch.cuda.Event(enable_timing=MARK == 1) for _ in range(8)]

    def step():
        n = state["i"]
        i = n % NI
        state["i"] += 1
        k = n % NS
        if AHEAD and n >= AHEAD and AHEAD <= NS:
            ev_out[(n - AHEAD) % NS].synchronize()
        e.stream.wait_event(ev_in[i])                     # this step's images (uploaded while the previous step computed)
        e.stream.wait_event(ev_out[k])                    # the output set about to be overwritten has been copied out
        e.mcs.check(e.lib.mcs_ctx_search_fence(e.ctx.h, 1))   # the search issued two calls ago (it read the set extracted three calls ago = this one) is complete
        b = job.sets[k]
        p = job.sets[(k - 1) % NS]                        # the set extracted in the previous call: patched, matched and sent home in this one
        job.cur = (k + 1) % NS
        t1 = time.perf_counter()
        job.extract(b, i)
        ev_free[i].record(e.stream)
        job.patch(1)                                      # host: wait for the previous batch's capture event only, recompute its rounding-tie rows, patch them
        job.exchange_end(p, job.exchange_begin(p))
        t2 = time.perf_counter()
        # The search is enqueued BEFORE the upload: the probed upload stream shares a hardware queue with the deferred matcher's stream (the least harmful pairing),
        # and a queue starts its packets in order — with the 1.3 ms upload in front, this step's lists started 1.3 ms late and finished right around the fence of step
        # n + 2: 1.60 ms per step in two runs of three, 1.8 - 2.1 in the third.  The upload has two steps of slack (MCS_E2E_ORDER=upload-first: the former order).
        upload_first = os.environ.get("MCS_E2E_ORDER", "") == "upload-first"
        if upload_first:
            upload((n + NI - 1) % NI)
        t3 = time.perf_counter()
        job.match(p)
        job.matched_set = p
        if not upload_first:
            upload((n + NI - 1) % NI)                     # the images of step n + NI - 1 travel while this and the following steps compute (NI = 2: the next step's)
        t4 = time.perf_counter()
        download_behind_search((k - 1) % NS)              # behind this call's greedy pass: the set leaves during the next step
        if MARK:
            marks[n % len(marks)].record(e.stream)
        t5 = time.perf_counter()
        for j, dt in enumerate((t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
            state["worst"][j] = max(state["worst"][j], dt * 1e3)
        state.setdefault("log", []).append((round((t1 - state.setdefault("t00", t1)) * 1e3, 2), round((t3 - t2) * 1e3, 2), round((t5 - t1) * 1e3, 2)))

    for ev in ev_free + ev_out:
        ev.record(e.stream)
    for i0 in range(NI - 1):
        upload(i0)
    # This leg is timed in its steady state.  Per process the runtime's H2D path goes through two settling phases, each ended by a 7-10 ms block of the host inside the
    # copy call four uploads after a device-wide synchronisation; until both are through, a step takes 1.93 instead of 1.60 ms (per-step log: MCS_E2E_DIAG=1).  Two
    # untimed rounds of steps, each closed by a synchronisation, put them in front of the clock.
    for _ in range(2):
        for _ in range(8):
            step()
        sync_all(e)
    elapsed = timed(e, step, warmup, steps, job.status)
    if os.environ.get("MCS_E2E_DIAG"):                    # where do slow steps come from: the spread of the per-step intervals on the GPU and of the host's enqueue time
        evs, host = [], []
        for _ in range(60):
            t0 = time.perf_counter()
            step()
            host.append((time.perf_counter() - t0) * 1e3)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(e.stream)
            evs.append(ev)
        torch.cuda.synchronize(e.dev)
        gaps = sorted(a.elapsed_time(b) for a, b in zip(evs, evs[1:]))
        sys.stderr.write("e2e diag: GPU step interval min %.3f median %.3f p90 %.3f max %.3f ms; host step() median %.3f max %.3f ms\n"
                         % (gaps[0], gaps[len(gaps) // 2], gaps[int(len(gaps) * 0.9)], gaps[-1], sorted(host)[len(host) // 2], max(host)))
        sys.stderr.write("e2e diag: host %s\n" % " ".join("%.2f" % h for h in host))
        sys.stderr.write("e2e diag: (index: start ms, upload ms, step ms) of every step over 2.3 ms or with a slow upload call: %s\n"
                         % " ".join("%d:%s/%s/%s" % ((j,) + x) for j, x in enumerate(state["log"]) if x[1] > 1.0 or x[2] > 2.3))
        lg = state["log"]
        sys.stderr.write("e2e diag: step starts (ms): %s\n" % " ".join("%.1f" % x[0] for x in lg))
        sys.stderr.write("e2e diag: slowest host call of a step (ms): extract %.2f upload %.2f match %.2f download %.2f\n" % tuple(state["worst"]))
    e.mcs.check(e.lib.mcs_ctx_join(e.ctx.h))
    n = state["i"]
    torch.cuda.synchronize(e.dev)
    feats = job.local_features()
    last = outs[(n - 2) % NS]                             # page-locked host copies of the set matched in the last call: (send = gathered array, nkp, kps, match, nmatch)
    job.matched_set = job.sets[(n - 2) % NS]
    checked = check_against_oracle(e, sp, job, host={"G": last[0][1], "kps": last[2][1], "match": last[3][1], "nmatch": last[4][1]}) if check else None
    h2d = job.imgs_np.nbytes
    d2h = sum(dst.numel() * dst.element_size() for _, dst in outs[0])

    def rate(fn, nbytes, reps=10):   # the copies alone, nothing else running
        torch.cuda.synchronize(e.dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(e.dev)
        return round(nbytes * reps / (time.perf_counter() - t0) / 1e9, 1)
    with torch.cuda.stream(cin):
        h2d_rate = rate(lambda: travel(job.d_imgs[0], h_img[0], wg_in, cin), h2d)
    with torch.cuda.stream(cout):
        d2h_rate = rate(lambda: [travel(dst, src, wg_out, cout) for src, dst in outs[0]], d2h)
    job.close()
    return {"value": round(feats * steps / elapsed / 1e6, 3), "unit": "Mfeatures/s", "ms_per_step": round(elapsed / steps * 1e3, 4), "oracle_check": checked,
            "oracle_checked": "the page-locked HOST copies of the last step's outputs: %s" % getattr(job, "checked", None),
            "h2d_bytes_per_step": int(h2d), "d2h_bytes_per_step": int(d2h), "h2d_GBps_alone": h2d_rate, "d2h_GBps_alone": d2h_rate,
            "copy_workgroups": {"h2d": wg_in or "runtime", "d2h": wg_out or "runtime"}, "upload_stream_queue_conflicts": upload_conflicts,
            "what": "host buffers at the boundary: images H2D from page-locked memory (three device buffers in turn, the runtime's SDMA copy on a copy stream), keypoints + "
                    "descriptor|mask blocks + counts + match arrays D2H to page-locked memory (mcs_copy_narrow on the context's result stream, behind the step's greedy "
                    "pass), overlapped with the neighbouring steps' kernels; rounding-tie rows patched on the host before the set's search is enqueued (in the loop); outputs leave one step late",
            "ties_patched_in_loop": bool(job.ties_in_loop), "ties_recomputed_on_the_host_in_loop": int(job.ties_patched)}


# ------------------------------------------------------------------------------------------------ oracle legs
def check_against_oracle(e, sp, job, host=None):
    """The timed output against the oracle, bit for bit: two multi-frames (every camera: keypoint records, descriptors, masks, counts) and the match
    indices of the (frame, keyframe) pairs they take part in — pair (1, 0) of the ring, or frames 0 and 1 against this rank's first two stored keyframes.
    `host`: the page-locked host copies of a buffer set (the e2e leg) instead of the device buffers."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    lay, rig, view = job.lay, e.rig, job.view
    do_db, masks_on = MODES[sp.mode]
    b = job.last()
    e.torch.cuda.synchronize(e.dev)
    src = host or {"G": b.G, "kps": b.kps, "match": b.match, "nmatch": b.nmatch}
    G = src["G"].cpu().numpy().reshape(view.images_total, lay.rows_img, lay.row_stride)
    local = (lambda f: f + 1) if job.ring else (lambda f: f)   # ring exchange (rank 0): global frame f is local frame f + 1 of the rank's array
    kps = src["kps"].cpu().numpy().view(np.uint8).reshape(lay.L, lay.cap, 28)
    match, nmatch = src["match"].cpu().numpy(), src["nmatch"].cpu().numpy()
    mine = {cf: i for i, cf in enumerate(job.slab)}   # (camera, frame) -> local image (keypoint records stay on the rank that extracted them)
    bad = []
    want = {}
    for f in ((1, 0) if (job.FT > 1 and (not job.ring or sp.F > 1)) else (0,)):
        d, m, v = rig.unpack_frame(view, G, local(f))
        want[f] = (d, m, v)
        for c in range(sp.ncam):
            ok_, od, om = O.Extractor(nfeatures=sp.nfeat, do_dBrief=do_db, learnMasks=masks_on)(e.synth.stream_image(f, c, job.cams[c], POOL),
                                                                                                 e.synth.mirror_mask(job.cams[c]), O.make_ocam(job.cams[c]))
            lo = c * lay.cap
            if not (int(v[lo:lo + lay.cap].sum()) == len(od) and (d[lo:lo + len(od)] == od).all() and (m[lo:lo + len(od)] == om).all()):
                bad.append("descriptors/masks/count of frame %d camera %d" % (f, c))
            if (c, f) in mine and not np.array_equal(kps[mine[(c, f)], :len(ok_)].reshape(-1), np.ascontiguousarray(ok_).view(np.uint8).reshape(-1)):
                bad.append("keypoint records of frame %d camera %d" % (f, c))
    pairs = 0
    if sp.D == 0 and e.rank == 0 and len(want) > 1:
        # pair (frame 1, frame 0) is set 1 of rank 0's ring call
        (d1, m1, v1), (d0, m0, v0) = want[1], want[0]
        ones = np.full_like(d1, 255)
        n, m12 = O.search_kf_kf(d1, m1 if masks_on else ones, v1, d0, m0 if masks_on else ones, v0, bool(masks_on), 0.9)
        got = match.reshape(sp.F, lay.rows_frame)[1]
        pairs += 1
        if not (n == int(nmatch[1]) and np.array_equal(got, m12)):
            bad.append("match indices of the pair (frame 1, frame 0)")
    if sp.D > 0 and job.nkf:
        # database sweep: this rank's first two stored keyframes against multi-frames 0 and 1 = pairs (f, k) of the sweep call
        got_m = match.reshape(job.FT, job.nkf, lay.rows_frame)
        got_n = nmatch.reshape(job.FT, job.nkf)
        for k in range(min(2, job.nkf)):
            db = job.db[k].cpu().numpy()
            dk, mk, vk = np.ascontiguousarray(db[:, :lay.desc_size]), np.ascontiguousarray(db[:, lay.desc_size:]), job.db_valid[k].cpu().numpy()
            for f in want:
                df, mf, vf = want[f]
                keep = np.flatnonzero(vf)
                ones_k, ones_f = np.full_like(dk, 255), np.full((len(keep), lay.desc_size), 255, np.uint8)
                n, mm = O.search_kf_f(dk, mk if masks_on else ones_k, vk, np.ascontiguousarray(df[keep]), np.ascontiguousarray(mf[keep]) if masks_on else ones_f,
                                      bool(masks_on), 0.9)
                full = np.full(lay.rows_frame, -1, np.int32)
                full[keep] = mm
                pairs += 1
                if not (n == int(got_n[f, k]) and np.array_equal(got_m[f, k], full)):
                    bad.append("match indices of the pair (frame %d, stored keyframe %d)" % (f, job.kfs[k]))
    for msg in bad:
        print("oracle check FAILED [%s]: %s" % (sp.tag, msg), file=sys.stderr)
    job.checked = {"multi_frames": len(want), "images": len(want) * sp.ncam, "pairs": pairs}
    return not bad


def orc_frame(orc, ncam, cap, f):
    """multi-frame f of the oracle pass as (per-camera counts, strided row positions over ncam * cap rows)"""
    n = [int(orc["nkp"][f * ncam + c]) for c in range(ncam)]
    return n, np.concatenate([c * cap + np.arange(n[c]) for c in range(ncam)])


def orc_pair(orc, ncam, cap, f, rows_frame):
    """the oracle's SearchByBoW(KF,KF) of stream multi-frame f against its predecessor (f = 0: the ring's pair (0, POOL - 1), row POOL of the pass) as the device
    lays it out: an index per strided query row (-1 none), and the match count"""
    fo = f if f > 0 else POOL
    _, pq = orc_frame(orc, ncam, cap, fo)
    _, pt = orc_frame(orc, ncam, cap, fo - 1)
    m12 = orc["match"][fo, :len(pq)]
    full = np.full(rows_frame, -1, np.int32)
    full[pq] = np.where(m12 >= 0, pt[np.maximum(m12, 0)], -1)
    return full, int(orc["nmatch"][fo])


def check_full(e, sp, job, orc):
    """Every multi-frame of the stream's pool and every (frame, predecessor) pair — the ring's (0, POOL - 1) included — as the oracle computed them (orc: the outputs of
    cpu_baseline's orc_extract_match_many_out pass) against the host copies of the set the headline loop matched last (job.snapshot): keypoint records, descriptors,
    masks, counts, match indices and match counts, bit for bit."""
    lay, rig, snap = job.lay, e.rig, job.snapshot
    ncam, cap = sp.ncam, lay.cap
    G = snap["G"].reshape(lay.images_total, lay.rows_img, lay.row_stride)
    kps = snap["kps"].view(np.uint8).reshape(lay.L, lay.cap, 28)
    match, nmatch = snap["match"].reshape(sp.F, lay.rows_frame), snap["nmatch"]
    mine = {cf: i for i, cf in enumerate(job.slab)}
    okps = orc["kps"].view(np.uint8).reshape(orc["nf"] * ncam, orc["cap"], 28)
    bad = []
    nf = min(POOL, job.FT)
    for f in range(nf):
        d, m, v = rig.unpack_frame(lay, G, f)
        for c in range(ncam):
            i, lo = f * ncam + c, c * cap
            n = int(orc["nkp"][i])
            if not (int(v[lo:lo + cap].sum()) == n and np.array_equal(d[lo:lo + n], orc["desc"][i, :n]) and np.array_equal(m[lo:lo + n], orc["mask"][i, :n])):
                bad.append("descriptors/masks/count of frame %d camera %d" % (f, c))
            if (c, f) in mine and not np.array_equal(kps[mine[(c, f)], :n], okps[i, :n]):
                bad.append("keypoint records of frame %d camera %d" % (f, c))
    pairs = 0
    for f in range(0 if job.FT == POOL else 1, nf):
        full, n = orc_pair(orc, ncam, cap, f, lay.rows_frame)
        pairs += 1
        if not (n == int(nmatch[f]) and np.array_equal(match[f], full)):
            bad.append("match indices of the pair (frame %d, frame %d)" % (f, (f - 1) % job.FT))
    for msg in bad[:20]:
        print("oracle check (full) FAILED [%s]: %s" % (sp.tag, msg), file=sys.stderr)
    return not bad, {"multi_frames": nf, "images": nf * ncam, "pairs": pairs}


def check_sweep(sp, orc, pt):
    """one point of the batch sweep: the raw outputs of the native host's LAST call (its F multi-frames and F pairs) against the oracle pass"""
    ncam, cap, F = sp.ncam, pt["cap"], pt["multi_frames_per_call"]
    rows = ncam * cap
    raw = pt.pop("_raw")
    nkp = raw["nkp"].reshape(F, ncam)
    kps, dsc, msk = raw["kps"].reshape(F, rows, 28), raw["desc"].reshape(F, rows, 32), raw["mask"].reshape(F, rows, 32)
    match, nmatch = raw["match"].reshape(F, rows), raw["nmatch"]
    okps = orc["kps"].view(np.uint8).reshape(orc["nf"] * ncam, orc["cap"], 28)
    for j in range(F):
        f = (pt["first_frame"] + j) % POOL
        for c in range(ncam):
            i, lo = f * ncam + c, c * cap
            n = int(orc["nkp"][i])
            if not (int(nkp[j, c]) == n and np.array_equal(kps[j, lo:lo + n], okps[i, :n]) and np.array_equal(dsc[j, lo:lo + n], orc["desc"][i, :n])
                    and np.array_equal(msk[j, lo:lo + n], orc["mask"][i, :n])):
                return False
        full, n = orc_pair(orc, ncam, cap, f, rows)
        if not (n == int(nmatch[j]) and np.array_equal(match[j], full)):
            return False
    return True


def run_batch_sweep(e, sp, points=(1, 2, 4, 8, 16, 32, 64)):
    """Throughput as a function of the batch: F multi-frames PER CALL through the boundary the reference has — host buffers in and out, both calls synchronous
    (the reference presents ONE multi-frame per call: src/cTracking.cpp:206-235, src/cMultiFrame.cpp:92-216).  The native host (host/frame_latency.cpp, `batch F`)
    stages the call's 3 F images, runs ONE mcs_extract_batch and ONE mcs_search_kf_kf over F (multi-frame, predecessor) pairs, steady clock around the call.
    The raw outputs of every point's last call are kept for the oracle check (main(): check_sweep against the CPU-baseline pass)."""
    import subprocess
    import tempfile
    mcs, synth = e.mcs, e.synth
    do_db, masks_on = MODES[sp.mode]
    NCAM, W, H, nfeat = sp.ncam, sp.W, sp.H, sp.nfeat
    host = os.path.join(ROOT, "multicol-slam_amd", "host", "frame_latency")
    if not os.path.exists(host):
        return {"error": "multicol-slam_amd/host/frame_latency not built (__graft_entry__.build())"}
    cams = [synth.lafida_cameras()[c % 3] if (W, H) == (754, 480) else synth.scaled_camera(synth.lafida_cameras()[c % 3], W, H) for c in range(NCAM)]
    d = tempfile.mkdtemp(prefix="mcs_sweep_")
    np.stack([_IMAGE_CACHE[(W, H, c, f)] if (W, H, c, f) in _IMAGE_CACHE else synth.stream_image(f, c, cams[c], POOL) for c in range(NCAM) for f in range(POOL)]).tofile(d + "/images.bin")
    np.stack([np.ascontiguousarray(synth.mirror_mask(cams[c])) for c in range(NCAM)]).tofile(d + "/masks.bin")
    open(d + "/cams.bin", "wb").write(bytes((mcs.Ocam * NCAM)(*[mcs.make_ocam(cams[c]) for c in range(NCAM)])))
    pts = []
    for F in points:
        calls = max(24, min(300, 1600 // F))
        open(d + "/cfg.txt", "w").write("ncam %d\nwidth %d\nheight %d\nnfeatures %d\nmode %d\nframes %d\nbatch %d\ncalls %d\nwarmup 12\nprestaged 1\ntopk 32\ndevice %d\nimages %s/images.bin\nmasks %s/masks.bin\n"
                                        "cams %s/cams.bin\nout %s/out\n" % (NCAM, W, H, nfeat, do_db + masks_on, POOL, F, calls, e.local, d, d, d, d))
        r = subprocess.run([host, d + "/cfg.txt"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            pts.append({"multi_frames_per_call": F, "error": r.stderr[-300:]})
            continue
        nat = json.loads(r.stdout.strip().splitlines()[-1])
        pt = {"multi_frames_per_call": F, "calls": calls, "features_per_call": nat["features_last"], "ms_per_call": nat["total_ms"]["median"], "ms_per_call_p99": nat["total_ms"]["p99"],
              "extract_ms": nat["extract_ms"]["median"], "match_ms": nat["match_ms"]["median"], "Mfeatures_per_s": round(nat["features_last"] / nat["total_ms"]["median"] / 1e3, 3),
              "ms_per_multi_frame": round(nat["total_ms"]["median"] / F, 4), "cap": nat["cap"], "first_frame": nat["first_frame"]}
        pt["_raw"] = {"nkp": np.fromfile(d + "/out.nkp", np.int32), "kps": np.fromfile(d + "/out.kps", np.uint8), "desc": np.fromfile(d + "/out.desc", np.uint8),
                      "mask": np.fromfile(d + "/out.mask", np.uint8), "match": np.fromfile(d + "/out.match", np.int32), "nmatch": np.fromfile(d + "/out.nmatch", np.int32)}
        pts.append(pt)
    import shutil
    shutil.rmtree(d, ignore_errors=True)
    return {"points": pts, "what": "F multi-frames per call, page-locked HOST buffers in (the images lie in page-locked memory as a grabber that owns its buffers delivers them) and out, extraction and SearchByBoW(KF,KF) both synchronous (native C++ host, steady clock "
                                   "around each call, median); one call = stage 3 F images, ONE mcs_extract_batch, ONE mcs_search_kf_kf over F pairs"}


def cpu_baseline(args, e, sp, job):
    """The oracle (kind 'port') timed on this box's host cores on a bounded sample of the same stream."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    synth = e.synth
    do_db, masks_on = MODES[sp.mode]
    NCAM, W, H, nfeat = sp.ncam, sp.W, sp.H, sp.nfeat
    nproc = os.cpu_count() or 1
    quota = nproc            # CPU time this process may actually use: cgroup v2 cpu.max (the GPU box grants 16 of its 256 hardware threads)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = max(1, min(nproc, int(round(int(q) / int(per)))))
    except (OSError, ValueError):
        pass
    nf = args.cpu_frames or max(48, 3 * quota)
    pool = [[_IMAGE_CACHE.get((W, H, c, f)) if (W, H, c, f) in _IMAGE_CACHE else synth.stream_image(f, c, job.cams[c], POOL) for c in range(NCAM)]
            for f in range(min(POOL, nf))]
    flat = [np.ascontiguousarray(pool[f % POOL][c]) for f in range(nf) for c in range(NCAM)]
    mk = [np.ascontiguousarray(synth.mirror_mask(job.cams[c])) for c in range(NCAM)]
    iptr = (C.c_void_p * len(flat))(*[a.ctypes.data for a in flat])
    mptr = (C.c_void_p * len(flat))(*[mk[i % NCAM].ctypes.data for i in range(len(flat))])
    ocs = (O.Ocam * len(flat))(*[O.make_ocam(job.cams[i % NCAM]) for i in range(len(flat))])
    prm = O.make_params(nfeatures=nfeat, do_dBrief=do_db, learnMasks=masks_on)
    nmatch = (C.c_int * nf)()
    secs = (C.c_double * 2)()
    L = O.lib()
    L.orc_extract_match_many.restype = C.c_long
    L.orc_extract_match_many.argtypes = [C.POINTER(O.Params), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_double, C.c_void_p, C.c_void_p]
    def one_pass(n_frames, threads):
        tot = L.orc_extract_match_many(C.byref(prm), n_frames, NCAM, iptr, W, H, W, mptr, ocs, threads, 0.9, nmatch, secs)
        return secs[0] + secs[1], secs[0], secs[1], tot
    # median of >= 20 repetitions after 3 warm-ups.  The warm-ups also pick the thread count (the quota, and 2x for SMT / oversubscription).
    cand = sorted({quota, min(nproc, 2 * quota)})
    warm = {t: one_pass(nf, t)[0] for t in cand}
    threads = min(warm, key=warm.get)
    one_pass(nf, threads)
    if len(cand) < 2:
        one_pass(nf, threads)
    reps = [one_pass(nf, threads) for _ in range(20)]
    walls = sorted(r[0] for r in reps)
    wall, se, sm, tot = sorted(reps, key=lambda r: r[0])[len(reps) // 2]
    per_frame = tot / nf
    # the reference's own threading: one thread per camera of a multi-frame (#pragma omp parallel for num_threads(nrCams), src/cMultiFrame.cpp:128), the
    # multi-frames one after the other, the matcher single-threaded — NCAM images in flight at any time.  One warm-up, median of 5.
    # one more pass, untimed, whose outputs leave: the in-run checks compare every multi-frame and pair of the stream's pool with the device's (check_full, the
    # batch sweep).  POOL + 1 multi-frames: the last one is multi-frame 0 again, so that its pair is the ring's (0, POOL - 1).
    nfo = POOL + 1
    ocap = nfeat + 4 * prm.nlevels
    orc = None
    if prm.descSize == 32:
        flat_o = [np.ascontiguousarray(_IMAGE_CACHE[(W, H, c, f % POOL)] if (W, H, c, f % POOL) in _IMAGE_CACHE else synth.stream_image(f % POOL, c, job.cams[c], POOL))
                  for f in range(nfo) for c in range(NCAM)]
        iptr_o = (C.c_void_p * len(flat_o))(*[a.ctypes.data for a in flat_o])
        mptr_o = (C.c_void_p * len(flat_o))(*[mk[i % NCAM].ctypes.data for i in range(len(flat_o))])
        ocs_o = (O.Ocam * len(flat_o))(*[O.make_ocam(job.cams[i % NCAM]) for i in range(len(flat_o))])
        orc = {"nf": nfo, "cap": ocap, "nkp": np.zeros(nfo * NCAM, np.int32), "kps": np.zeros((nfo * NCAM, ocap, 7), np.float32), "desc": np.zeros((nfo * NCAM, ocap, 32), np.uint8),
               "mask": np.zeros((nfo * NCAM, ocap, 32), np.uint8), "match": np.full((nfo, NCAM * ocap), -1, np.int32), "nmatch": np.zeros(nfo, np.int32)}
        L.orc_extract_match_many_out.restype = C.c_long
        L.orc_extract_match_many_out.argtypes = L.orc_extract_match_many.argtypes + [C.c_void_p] * 5
        L.orc_extract_match_many_out(C.byref(prm), nfo, NCAM, iptr_o, W, H, W, mptr_o, ocs_o, threads, 0.9, orc["nmatch"].ctypes.data, secs, orc["nkp"].ctypes.data, orc["kps"].ctypes.data,
                                     orc["desc"].ctypes.data, orc["mask"].ctypes.data, orc["match"].ctypes.data)
    nf_f = max(4, min(nf, 12))
    one_pass(nf_f, NCAM)
    rf = sorted((one_pass(nf_f, NCAM) for _ in range(5)), key=lambda r: r[0])[2]
    faithful = {"value": round(rf[3] / nf_f * (nf_f - 1) / rf[0] / 1e6, 4), "unit": "Mfeatures/s", "cores": NCAM,
                "ms_per_multi_frame": round(rf[0] / nf_f * 1e3, 2),
                "sample": "%d multi-frames one after the other on %d threads (extraction: one thread per camera, the reference's threading; the frame pairs of the "
                          "matcher share the same threads): extract %.2fs + match %.2fs, median of 5 passes after a warm-up" % (nf_f, NCAM, rf[1], rf[2])}
    # The REFERENCE-COMPILED figure: oracle/_ref = the reference's own src/mdBRIEFextractorOct.cpp, src/cMultiFrame.cpp, src/cORBmatcher.cpp ... built here,
    # unmodified, against oracle/cvshim (OpenCV's image primitives are the oracle's restatements: OpenCV itself is not in the image).  Single thread (that build
    # has no OpenMP): cMultiFrame's constructor per multi-frame + cORBmatcher::SearchByBoW(KF,KF) against the previous keyframe; and with the reference's
    # threading for the extraction — one thread per camera, each running the reference's extractor — the matcher single-threaded as in the reference.
    refc = None
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libmcs_ref.so")
    if os.path.exists(ref_so) and NCAM == 3:
        try:
            import threading
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import ref_compare as R
            import ref_scene
            import test_io_formats as T
            io = importlib.import_module("multicol-slam_amd.io")
            S = ref_scene.RefScene(job.cams[:NCAM], mk, [io.cayley2hom(c) for c in T.CAYLEY], None, so_path=ref_so, nfeatures=nfeat, do_dBrief=do_db, learnMasks=masks_on)
            nr = 4
            t_ext, feats = [], []
            for f in range(nr):
                t0 = time.perf_counter()
                fid = S.add_frame([flat[f * NCAM + c] for c in range(NCAM)], 0.04 * f, np.eye(4))
                t_ext.append(time.perf_counter() - t0)
                feats.append(S.L.rs_frame_total(S.h, fid))
            kfs = [S.make_keyframe(f) for f in range(nr)]
            for f in range(nr):
                S.set_mappoints(True, kfs[f], np.ones(feats[f], np.uint8), base=100000 * f, ref_kf=kfs[f])
            t_m = []
            for f in range(1, nr):
                t0 = time.perf_counter()
                S._ids(S.L.rs_bow_kf_kf, feats[f], kfs[f], kfs[f - 1], 0.9)
                t_m.append(time.perf_counter() - t0)
            S.close()
            t3 = []
            for f in range(nr):
                th = [threading.Thread(target=R.run_ref, args=(flat[f * NCAM + c], mk[c], job.cams[c]), kwargs=dict(nfeatures=nfeat, do_dBrief=do_db, learnMasks=masks_on)) for c in range(NCAM)]
                t0 = time.perf_counter()
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
                t3.append(time.perf_counter() - t0)
            ext1, ext3, mt, fpm = float(np.median(t_ext)), float(np.median(t3)), float(np.median(t_m)), float(np.mean(feats))
            refc = {"kind": "reference", "single_thread": {"value": round(fpm / (ext1 + mt) / 1e6, 5), "unit": "Mfeatures/s", "cores": 1, "extract_ms_per_multi_frame": round(ext1 * 1e3, 1),
                                                            "match_ms_per_pair": round(mt * 1e3, 1)},
                    "one_thread_per_camera": {"value": round(fpm / (ext3 + mt) / 1e6, 5), "unit": "Mfeatures/s", "cores": NCAM, "extract_ms_per_multi_frame": round(ext3 * 1e3, 1),
                                              "match_ms_per_pair": round(mt * 1e3, 1)},
                    "sample": "%d multi-frames: cMultiFrame::cMultiFrame (src/cMultiFrame.cpp:92-216) and cORBmatcher::SearchByBoW(KF,KF) (src/cORBmatcher.cpp:885-966) of the "
                              "reference's own sources compiled here (oracle/_ref), medians; threads = Python threads around the reference's extractor (the GIL is released)" % nr}
        except Exception as ex:   # this side measurement is optional; the error is reported, not hidden
            refc = {"error": "%s: %s" % (type(ex).__name__, str(ex)[:200])}
    return {"_oracle_outputs": orc, "reference_compiled": refc, "reference_threading": faithful, "value": round(per_frame * (nf - 1) / wall / 1e6, 4), "unit": "Mfeatures/s", "cores": threads, "kind": "port",
            "repetitions": len(reps), "warmups": 3, "wall_s_min_median_max": [round(walls[0], 3), round(wall, 3), round(walls[-1], 3)],
            "sample": "%d multi-frames (%d images) of the same synthetic stream: oracle extract (%s) %.2fs + SearchByBoW(KF,KF) vs previous frame %.2fs wall, "
                      "OpenMP over images/frames on %d threads (cgroup CPU quota of this box: %d of %d hardware threads; thread count picked by the warm-ups from quota and "
                      "2x quota); MEDIAN of 20 passes after 3 warm-ups"
                      % (nf, nf * NCAM, sp.mode, se, sm, threads, quota, nproc),
            "cpu_model": cpu_model(), "cpu_quota": quota, "nproc": nproc}


def run_latency(e, sp, calls=300, py_calls=200):
    """ONE multi-frame per call — the reference's own unit of work (cTracking builds one cMultiFrame per grabbed image set and tracks it, src/cTracking.cpp:206-235).
    Per call: mcs_extract_batch of the rig's images with HOST buffers in and out (synchronous), then SearchByBoW(KF,KF) of that multi-frame against the one before it
    (mcs_search_kf_kf, host buffers, synchronous).  Measured twice: by the native C++ program (multicol-slam_amd/host/frame_latency: page-locked buffers, no Python in
    the loop — the figure a C++ tracker sees) and by a Python / ctypes loop over the same entry points (numpy buffers).  The last native call is checked against the
    oracle: keypoints, descriptors, masks, counts, match indices."""
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    mcs, synth = e.mcs, e.synth
    do_db, masks_on = MODES[sp.mode]
    NCAM, W, H, nfeat = sp.ncam, sp.W, sp.H, sp.nfeat
    cams = [synth.lafida_cameras()[c % 3] if (W, H) == (754, 480) else synth.scaled_camera(synth.lafida_cameras()[c % 3], W, H) for c in range(NCAM)]
    frames = 8
    imgs = [[np.ascontiguousarray(synth.stream_image(f, c, cams[c], POOL)) for f in range(frames)] for c in range(NCAM)]
    masks = [np.ascontiguousarray(synth.mirror_mask(cams[c])) for c in range(NCAM)]
    out = {"unit_of_work": "one %d-camera %dx%d multi-frame per call: %s extraction (N = %d) with host buffers in and out + SearchByBoW(KF,KF) against the previous multi-frame, both synchronous"
                           % (NCAM, W, H, sp.mode, nfeat)}
    host = os.path.join(ROOT, "multicol-slam_amd", "host", "frame_latency")
    ok = None
    if os.path.exists(host):
        d = os.environ.get("MCS_KEEP_LATENCY_DIR") or tempfile.mkdtemp(prefix="mcs_latency_")   # (kept when named: tools/latency_trace.sh reruns the program under the profiler)
        os.makedirs(d, exist_ok=True)
        np.stack([imgs[c][f] for c in range(NCAM) for f in range(frames)]).tofile(d + "/images.bin")
        np.stack(masks).tofile(d + "/masks.bin")
        open(d + "/cams.bin", "wb").write(bytes((mcs.Ocam * NCAM)(*[mcs.make_ocam(cams[c]) for c in range(NCAM)])))
        open(d + "/cfg.txt", "w").write("ncam %d\nwidth %d\nheight %d\nnfeatures %d\nmode %d\nframes %d\ncalls %d\nwarmup 20\ntopk 32\ndevice %d\nimages %s/images.bin\nmasks %s/masks.bin\n"
                                        "cams %s/cams.bin\nout %s/out\n" % (NCAM, W, H, nfeat, do_db + masks_on, frames, calls, e.local, d, d, d, d))
        r = subprocess.run([host, d + "/cfg.txt"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            out["native"] = {"error": r.stderr[-300:]}
            ok = False
        else:
            nat = json.loads(r.stdout.strip().splitlines()[-1])
            cap, fl = nat["cap"], nat["last_frame"]
            rows = NCAM * cap
            nkp = np.fromfile(d + "/out.nkp", np.int32)
            kps = np.fromfile(d + "/out.kps", np.uint8).reshape(rows, 28)
            dsc, msk = np.fromfile(d + "/out.desc", np.uint8).reshape(rows, 32), np.fromfile(d + "/out.mask", np.uint8).reshape(rows, 32)
            match = np.fromfile(d + "/out.match", np.int32)
            # the oracle on the same two multi-frames, laid out like the native program's sets (camera blocks of `cap` rows, rows past a camera's count invalid)
            want = {}
            for f in (fl, (fl - 1) % frames):
                D, M, V = np.zeros((rows, 32), np.uint8), np.zeros((rows, 32), np.uint8), np.zeros(rows, np.uint8)
                K = []
                for c in range(NCAM):
                    k_, d_, m_ = O.Extractor(nfeatures=nfeat, do_dBrief=do_db, learnMasks=masks_on)(imgs[c][f], masks[c], O.make_ocam(cams[c]))
                    D[c * cap:c * cap + len(d_)], M[c * cap:c * cap + len(d_)], V[c * cap:c * cap + len(d_)] = d_, m_, 1
                    K.append(k_)
                want[f] = (D, M, V, K)
            D1, M1, V1, K1 = want[fl]
            D0, M0, V0, _ = want[(fl - 1) % frames]
            ones = np.full_like(D1, 255)
            n, m12 = O.search_kf_kf(D1, M1 if masks_on else ones, V1, D0, M0 if masks_on else ones, V0, bool(masks_on), 0.9)
            ok = (all(int(nkp[c]) == len(K1[c]) for c in range(NCAM)) and all(np.array_equal(kps[c * cap:c * cap + len(K1[c])].reshape(-1), np.ascontiguousarray(K1[c]).view(np.uint8).reshape(-1)) for c in range(NCAM))
                  and all(np.array_equal(dsc[c * cap:c * cap + nkp[c]], D1[c * cap:c * cap + nkp[c]]) and np.array_equal(msk[c * cap:c * cap + nkp[c]], M1[c * cap:c * cap + nkp[c]]) for c in range(NCAM))
                  and n == nat["matches_last"] and np.array_equal(match, m12))
            nat["oracle_check"] = bool(ok)
            nat["what"] = ("native C++ host (multicol-slam_amd/host/frame_latency.cpp): page-locked staging and result arrays (the library writes the valid rows into them with one launch), the rig's mirror "
                           "masks resident on the device (mcs_extractor_set_masks), the launch sequence replayed from a hipGraph; %d timed calls after 20 warm-up calls, steady clock around each call" % calls)
            out["native"] = nat
            out["median_ms"], out["p99_ms"] = nat["total_ms"]["median"], nat["total_ms"]["p99"]
            out["features_per_call"] = nat["features_last"]
            out["Mfeatures_per_s_at_batch_1"] = round(nat["features_last"] / nat["total_ms"]["median"] / 1e3, 3)
    else:
        out["native"] = {"error": "multicol-slam_amd/host/frame_latency not built (__graft_entry__.build())"}
    # the same two entry points from Python (ctypes, numpy buffers — what the -m gpu tests and frontend.py do)
    ctx = mcs.Context(e.local)
    ex = mcs.Extractor(ctx, W, H, max_batch=NCAM, nfeatures=nfeat, do_dBrief=do_db, learnMasks=masks_on)
    oc = [mcs.make_ocam(c) for c in cams]
    cap = ex.cap
    rows = NCAM * cap
    bufs = []
    for _ in range(2):
        bufs.append(dict(desc=np.zeros((rows, 32), np.uint8), mask=np.zeros((rows, 32), np.uint8), valid=np.zeros(rows, np.uint8)))
    m12, nm, fb = np.full(rows, -1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    te, tm = [], []
    for it in range(20 + py_calls):
        f = it % frames
        cur, prev = bufs[it & 1], bufs[(it & 1) ^ 1]
        t0 = time.perf_counter()
        res = ex.extract_host([imgs[c][f] for c in range(NCAM)], masks, oc, want_rays=True)
        for c in range(NCAM):
            k = len(res[c][0])
            cur["desc"][c * cap:c * cap + k], cur["mask"][c * cap:c * cap + k] = res[c][1], res[c][2]
            cur["valid"][c * cap:c * cap + k], cur["valid"][c * cap + k:(c + 1) * cap] = 1, 0
        t1 = time.perf_counter()
        if it > 0:
            q = mcs.DescSet(mcs.np_ptr(cur["desc"]), mcs.np_ptr(cur["mask"]) if masks_on else None, mcs.np_ptr(cur["valid"]), None, rows, 32)
            t = mcs.DescSet(mcs.np_ptr(prev["desc"]), mcs.np_ptr(prev["mask"]) if masks_on else None, mcs.np_ptr(prev["valid"]), None, rows, 32)
            mcs.check(e.lib.mcs_search_kf_kf(ctx.h, 1, C.byref(q), 0, C.byref(t), 0, 32, 0.9, 32, 0, mcs.np_ptr(m12), mcs.np_ptr(nm), mcs.np_ptr(fb)))
        t2 = time.perf_counter()
        if it >= 20:
            te.append(1e3 * (t1 - t0)); tm.append(1e3 * (t2 - t1))
    tot = np.array(te) + np.array(tm)
    out["python_ctypes"] = {"calls": py_calls, "extract_ms_median": round(float(np.median(te)), 4), "match_ms_median": round(float(np.median(tm)), 4),
                            "total_ms": {"median": round(float(np.median(tot)), 4), "p99": round(float(np.percentile(tot, 99)), 4)},
                            "what": "the same two calls from Python (Extractor.extract_host over the extractor's page-locked buffers, the per-image results copied out into numpy arrays; ctypes)"}
    ex.close()
    ctx.close()
    out["oracle_check"] = ok
    return out


def secondary_args(args, **kw):
    a = argparse.Namespace(**vars(args))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def main():
    args = parse()
    if args.dry_run:
        sys.exit(dry_run(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    e = setup(args)
    if args.exchange == "nccl1":
        force_exchange_world1(e)
    sp = Spec(args, e.world)
    # a plain run times the headline and nothing else; the oracle check (--check) and everything below that is not the headline need --full
    check = (args.full or args.check) and not args.no_check
    job, out = run_job(e, sp, args, args.steps, args.warmup, want_roofline=args.full, check=check, dump=args.dump_outputs)
    headline = args.workload == "stream" and args.mode == "mdbrief" and not (args.ncam or args.width or args.height or args.nfeatures or args.keyframes >= 0
                                                                               or args.frames or args.exchange != "auto")
    out["cpu_baseline"] = None   # filled in LAST (below): the oracle's OpenMP threads keep spinning for a while after their last parallel region, on the same 16 CPUs
                                 # the host thread needs for the legs that follow (measured: the e2e leg right behind the baseline 2.36 instead of 1.66 ms per step)
    job.close()
    checks = [out.get("oracle_check")]
    if e.world == 1 and args.e2e_sweep:
        out["e2e_sweep"] = {}
        for item in args.e2e_sweep.split(","):
            os.environ["MCS_E2E_H2D"], os.environ["MCS_E2E_D2H"] = item.split(":")
            r = run_e2e(e, sp, args.steps, args.warmup, check)
            checks.append(r["oracle_check"])
            out["e2e_sweep"][item] = {k: r[k] for k in ("value", "ms_per_step", "oracle_check", "h2d_GBps_alone", "d2h_GBps_alone")}
    elif e.world == 1 and headline and args.full and not args.no_secondary:
        # further legs of the default run, each bounded: host buffers at the boundary (configs[1] and [2]); the matcher-dominated BASELINE configs[2]; the
        # reference's shipped settings; the N > 1 code path at world size 1 over RCCL
        s2 = min(args.steps, 10)
        out["e2e"] = run_e2e(e, sp, args.steps, args.warmup, check)
        checks.append(out["e2e"]["oracle_check"])
        # the PCIe-inclusive rate of the same step (host buffers in and out), beside the resident-input `value`; in `config` so that it is among the keys the driver parses
        out["config"]["host_boundary_e2e"] = {k: out["e2e"][k] for k in ("value", "unit", "ms_per_step", "oracle_check")}
        sec = []
        for a in (secondary_args(args, workload="db", frames=16), secondary_args(args, mode="orb", nfeatures=400)):
            j2, o2 = run_job(e, Spec(a, e.world), a, s2, 2, check=check)
            j2.close()
            sec.append({k: o2[k] for k in ("metric", "value", "unit", "steps", "ms_per_step", "config", "roofline", "oracle_check") if k in o2})
            checks.append(o2.get("oracle_check"))
        a = secondary_args(args, workload="db", frames=16)
        sec[0]["e2e"] = run_e2e(e, Spec(a, e.world), s2, 2, check)
        checks.append(sec[0]["e2e"]["oracle_check"])
        out["secondary"] = sec
        out["latency"] = run_latency(e, sp)
        checks.append(out["latency"]["oracle_check"])
        if not args.no_cpu_baseline:   # (its oracle check needs the CPU-baseline pass)
            out["batch_sweep"] = run_batch_sweep(e, sp)
        try:   # a one-rank RCCL group: the code path of the N > 1 runs (the driver's SCALE run) on this box's own RCCL
            force_exchange_world1(e)
            j3, o3 = run_job(e, sp, args, s2, 2, want_roofline=False, check=check)
            j3.close()
            out["exchange_world1"] = {k: o3[k] for k in ("value", "unit", "steps", "ms_per_step", "oracle_check") if k in o3}
            out["exchange_world1"]["parallelism"] = o3["config"]["parallelism"]
            out["exchange_world1"]["what"] = ("the N > 1 step of configs[1] (send buffer -> asynchronous point-to-point batch on RCCL, at world size 1 a self send / receive of "
                                              "this rank's own camera blocks -> wait -> row flags -> matching one step late, three buffer sets) at world size 1, backend "
                                              "nccl; the sweeps' all_gather_into_tensor form runs at world size 1 in tests/test_gpu_bench_jobs.py")
            checks.append(o3.get("oracle_check"))
        except Exception as ex:   # an environment without a usable RCCL is reported, not hidden; a wrong RESULT is a failed check above
            out["exchange_world1"] = {"error": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
        e.exchange = False
    if e.rank == 0 and e.world == 1 and headline and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline(args, e, sp, job)
        orc = cpu.pop("_oracle_outputs", None)
        if check and orc is not None and getattr(job, "snapshot", None) is not None:
            # the widened check: every multi-frame and pair of the CPU sample against the set the headline's timed loop matched last
            ok_full, counts = check_full(e, sp, job, orc)
            out["oracle_check_full"] = bool(ok_full)
            out["oracle_check"] = bool(out.get("oracle_check")) and bool(ok_full)
            out["config"]["oracle_checked"] = dict(counts, first_pass=out["config"].get("oracle_checked"),
                                                   what="all multi-frames and (frame, predecessor) pairs of the CPU-baseline sample against the set the timed loop matched last")
            checks.append(bool(ok_full))
        sw = out.get("batch_sweep")
        if isinstance(sw, dict) and "points" in sw:
            # where the >= 50x target is crossed: against the all-quota CPU figure, and against that figure scaled linearly to every hardware thread of the host
            for pt in sw["points"]:
                if "_raw" in pt:
                    if check and orc is not None:
                        pt["oracle_check"] = bool(check_sweep(sp, orc, pt))
                        checks.append(pt["oracle_check"])
                    else:
                        pt.pop("_raw")
                        pt["oracle_check"] = None
                if "Mfeatures_per_s" in pt:
                    pt["vs_cpu_all_quota"] = round(pt["Mfeatures_per_s"] / cpu["value"], 1)
            full_host = cpu["value"] * cpu["nproc"] / max(cpu["cpu_quota"], 1)
            ok_pts = [pt for pt in sw["points"] if "Mfeatures_per_s" in pt]
            sw["cpu_all_quota_Mfeatures_per_s"] = cpu["value"]
            sw["cpu_scaled_to_all_hardware_threads_Mfeatures_per_s"] = round(full_host, 4)
            sw["smallest_batch_at_50x_cpu_quota"] = next((pt["multi_frames_per_call"] for pt in ok_pts if pt["Mfeatures_per_s"] >= 50 * cpu["value"]), None)
            sw["smallest_batch_at_50x_cpu_scaled_to_all_hardware_threads"] = next((pt["multi_frames_per_call"] for pt in ok_pts if pt["Mfeatures_per_s"] >= 50 * full_host), None)
            out["config"]["batch_sweep_Mfeatures_per_s"] = {str(pt["multi_frames_per_call"]): pt["Mfeatures_per_s"] for pt in ok_pts}
        out["cpu_baseline"] = cpu
        out["speedup_vs_cpu_all_cores"] = round(out["value"] / cpu["value"], 2)
        out["speedup_vs_cpu_reference_threading"] = round(out["value"] / cpu["reference_threading"]["value"], 2)
        if isinstance(out.get("latency"), dict):   # the same unit of work on the host: one multi-frame at a time with the reference's threading
            out["latency"]["cpu_reference_threading_ms_per_multi_frame"] = cpu["reference_threading"]["ms_per_multi_frame"]
            if isinstance(cpu.get("reference_compiled"), dict) and "one_thread_per_camera" in cpu["reference_compiled"]:
                rc = cpu["reference_compiled"]["one_thread_per_camera"]
                out["latency"]["reference_compiled_ms_per_multi_frame"] = round(rc["extract_ms_per_multi_frame"] + rc["match_ms_per_pair"], 1)
    failed = check and e.rank == 0 and any(c is False for c in checks)
    if e.dist.is_initialized():
        e.dist.barrier()
        e.dist.destroy_process_group()
    if e.rank == 0:
        # the JSON line is the LAST line of stdout: RCCL prints its version banner through C stdio (NCCL_DEBUG=VERSION on these boxes), flush that first
        sys.stdout.flush()
        try:
            C.CDLL(None).fflush(None)
        except (OSError, AttributeError):
            pass
        print(json.dumps(out))
        sys.stdout.flush()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
