#!/usr/bin/env python3
"""bench.py -- decoded Mpixels/s of the MI355X DIINN implicit-decoder path.

Contract (driver):  python bench.py --gpus N --steps K --warmup W
  N > 1 is launched by the driver as
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
  The bare form `python bench.py --gpus N` (no launcher, WORLD_SIZE unset) starts exactly that command as a child
  process before anything touches the GPU and relays rank 0's line (_self_launch_if_bare).

Default workload (BASELINE.json configs[1], "c2"): 256x256 LR encoder features, x4 decode
-> 1024x1024 HR, fp32, synthetic features (seeded N(0,1)) and synthetic weights drawn from the
reference decoder's default-init distribution (synth.py).  A *step* is one full pass of the hot
path over one batch: feature hand-off (N>1) + P precompute (hoisted 3x3 conv) + fused decode
kernel, inputs already resident in HBM on the rank that holds the encoder output.

--workload {c1,c2,c3,tgt,c4,c5} selects another BASELINE config (tgt = the north-star target
1024^2 -> 4096^2).  --scaling weak (default): every GPU decodes one whole workload image (the LR
map grows to (H*N) x W, one row band per rank).  --scaling strong: ONE workload image is split
into N row bands (BASELINE configs c3/c4: "tiled across 2 then 4", "8 GPUs tile-sharded").
Either way each rank holds band-sized buffers only and receives its feature rows (+1-row halo)
point-to-point from rank 0 over RCCL/xGMI; with one rank the same code path runs with an empty
exchange.  Outputs stay sharded; --gather additionally times assembling the image on rank 0.

A plain run does only what the headline needs: set up, warm up, time the --steps steps, write the
timed output if --dump-outputs DIR is given, print the line.  --full adds everything else the
benchmark measures or checks: the timed output against the CPU oracle on a few HR row bands
("checked"; the run fails if that is out of tolerance), the split-bf16, target-shape, side,
whole-model and strong-scaling legs, the in-run HBM traffic passes and the CPU baseline.

--dump-outputs DIR: after the timed steps each rank writes the HR output of the last timed step
(what a caller of the path receives; its own band when N > 1) as DIR/output.npy (float32; N > 1:
DIR/output_rank<r>.npy).  An output above the 64 MB budget is cut to a fixed, seeded sample of
whole HR rows.  Inputs and weights are seeded, so the same arguments give the same inputs.

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for every field).
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import socket
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")



def _self_launch_if_bare() -> None:
    """``python bench.py --gpus N`` with N > 1 and NO launcher around it (WORLD_SIZE unset): start the N ranks ourselves.

    The contract's form is ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N``; the only
    driver command on record is the bare N = 1 one, so the bare form with N > 1 must not be a lost 8-GPU lease.  This
    process has imported nothing but the standard library at this point (torch is imported BELOW this call) and never
    touches HIP: it starts that very command as a CHILD in a process group of its own, relays the child's stdout -- rank 0's
    one JSON line -- to its own stdout (anything else a launcher prints there goes to stderr), and exits with the child's
    code.  --watchdog: the child GROUP is killed and the exit code is 124.  Nothing is ever re-executed in place.
    (The reference has nothing to mirror here: /root/reference/benchmarks.py:13 runs one device.)"""
    if __name__ != "__main__" or "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--gpus", type=int, default=1)
    pre.add_argument("--watchdog", type=int, default=int(os.environ.get("DIINN_BENCH_WATCHDOG", "1500")))
    known, _ = pre.parse_known_args()
    if known.gpus <= 1:
        return
    import signal
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={known.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    sys.stderr.write(f"bench.py: --gpus {known.gpus} without a launcher (WORLD_SIZE unset): starting the ranks as a child: "
                     f"{' '.join(cmd)}\n")
    sys.stderr.flush()
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT, start_new_session=True)

    def _kill_group():
        try:
            os.killpg(child.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass

    expired = threading.Event()
    if known.watchdog > 0:
        def _expired():
            expired.set()
            sys.stderr.write(f"bench.py: the {known.gpus}-rank child is still running after {known.watchdog} s: killing its "
                             f"process group, exiting with code 124\n")
            sys.stderr.flush()
            _kill_group()
        wd = threading.Timer(known.watchdog, _expired)
        wd.daemon = True
        wd.start()
    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, lambda *_: (_kill_group(), os._exit(128 + 15)))
    try:
        for line in child.stdout:
            out = sys.stdout if line.startswith("{") else sys.stderr
            out.write(line)
            out.flush()
        code = child.wait()
    finally:
        _kill_group()                                     # no rank outlives this process
    sys.exit(124 if expired.is_set() else (code if code >= 0 else 128 - code))


_self_launch_if_bare()

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# BASELINE.json configs (LR map, HR size); "tgt" is the north_star target shape
WORKLOADS = {
    "c1": ((48, 48), (96, 96), "c1: 48x48 LR, x2 decode -> 96x96 HR"),
    "c2": ((256, 256), (1024, 1024), "c2: 256x256 LR encoder features, x4 decode -> 1024x1024 HR"),
    "c3": ((512, 512), (2048, 2048), "c3: 512x512 LR, x4 decode -> 2048x2048 HR"),
    "tgt": ((1024, 1024), (4096, 4096), "north-star target: 1024x1024 LR, x4 decode -> 4096x4096 HR"),
    "c4": ((1024, 1024), (8192, 8192), "c4: 1024x1024 LR, x8 decode -> 8192x8192 HR"),
    "c5": ((720, 1280), (2376, 4224), "c5: 720x1280 LR, x3.3 decode -> 2376x4224 HR"),
}
_M = "decoded Mpixels/sec (DIINN implicit decoder, %s)"
METRIC = {"c1": _M % "x2 on 48^2 LR", "c2": _M % "x4 on 256^2 LR", "c3": _M % "x4 on 512^2 LR",
          "tgt": _M % "x4 on 1024^2 LR", "c4": _M % "x8 on 1024^2 LR", "c5": _M % "x3.3 on 720x1280 LR"}
FLOP_DECODE_PER_PX = 789_504.0        # 3 stacked 512x256 layers + Q0 + head, 2*MAC
FLOP_P_PER_CELL = 1_179_648.0         # hoisted 3x3 conv 64 -> 1024, 2*MAC
PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0        # MI355X_MICROARCH.md: ~2.5 PF dense bf16 (only for --compute bf16*)
# parity bound of the post-run check: f32 = north_star's 1e-4; bf16 restated (SURVEY §8 d4 / DESIGN §3.4)
CHECK_TOL = {"f32": (1e-4, True), "bf16": (2e-3, False), "bf16_full": (3e-3, False), "bf16x3": (1e-4, True)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c2")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: one workload image per GPU; strong: one image split into N row bands")
    ap.add_argument("--sin", choices=["accurate", "hw", "hw_reduced"], default=os.environ.get("DIINN_SIN", "default"),
                    help="sine evaluation of the synthesis branch (default: the library default, hw_reduced)")
    ap.add_argument("--compute", choices=["f32", "bf16", "bf16_full", "bf16x3"], default="f32",
                    help="arithmetic of the per-pixel layers; f32 is the reference's precision and the only "
                         "valid headline (bf16 is BASELINE config 5's optional path, 2e-3 relative; bf16x3 = split "
                         "bf16, three bf16 MFMA products per term, held to f32's 1e-4)")
    ap.add_argument("--no-split", action="store_true", help="skip the split-bf16 side leg of a --full run")
    ap.add_argument("--dist-mode", choices=["halo", "bcast"], default="halo")
    ap.add_argument("--gather", action="store_true", help="also time assembling the image on rank 0 (reported "
                                                           "as gather_ms, never part of value)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default=os.environ.get("DIINN_BENCH_BACKEND", "nccl"),
                    help="nccl = RCCL over xGMI (one rank per GPU).  gloo: messages staged through pinned host memory; "
                         "with DIINN_BENCH_ONE_DEVICE=1 all ranks share cuda:0, which is how every N>1 branch is "
                         "exercised on a one-GPU box (RCCL refuses two ranks on one device) -- a test transport, "
                         "its timings mean nothing.  DIINN_BENCH_BACKEND sets the default, so that the driver's literal "
                         "command line can be run on such a box")
    ap.add_argument("--dist-timeout", type=int, default=int(os.environ.get("DIINN_BENCH_DIST_TIMEOUT", "300")),
                    help="N>1: seconds a collective of the process group may wait for a peer before the rank fails")
    ap.add_argument("--watchdog", type=int, default=int(os.environ.get("DIINN_BENCH_WATCHDOG", "1500")),
                    help="seconds after which a run that has not finished is ended with exit code 124 (0: off): a hung "
                         "rank or hand-off exits non-zero inside the driver's budget -- the process is ENDED, never re-executed")
    ap.add_argument("--no-strong", action="store_true", help="N>1: skip the strong-scaling legs")
    ap.add_argument("--strong-legs", default=None, help="N>1: comma-separated workloads of the strong-scaling legs "
                                                          "(default by N: tgt+c3 at 2/4, tgt+c4 at 8)")
    ap.add_argument("--strong-steps", type=int, default=3)
    ap.add_argument("--no-target", action="store_true", help="N=1: skip the two extra steps at the target shape")
    ap.add_argument("--no-side-legs", action="store_true", help="N=1: skip the c5 fp32 / c5 bf16_full / c1 side legs")
    ap.add_argument("--no-traffic", action="store_true", help="N=1 c2 fp32: skip the two rocprofv3 --pmc child runs that measure "
                                                              "roofline.traffic (the committed measurement is reported, labelled)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: the oracle check, the extra legs, the traffic passes, "
                         "the CPU baseline (each --no-* option above then turns one of them off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the output of the last timed step as DIR/output.npy (N > 1: output_rank<r>.npy per rank)")
    return ap.parse_args()


DUMP_BUDGET_BYTES = 64_000_000          # all dumped arrays together, .npy headers included


def dump_rows(hu_rows, row_bytes, budget):
    """HR rows (band-relative indices) to dump: all of them if they fit ``budget`` bytes, else a fixed, seeded, sorted
    sample of whole rows that does."""
    import numpy as np
    keep = max(1, (budget - 4096) // row_bytes)
    if hu_rows <= keep:
        return None
    return np.sort(np.random.default_rng(2024).choice(hu_rows, size=keep, replace=False))


def dump_outputs(directory, out_band, rank, world):
    """The timed path's output (this rank's band, (B, 3, rows, WU) float32) -> directory/<name>.npy."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    out = out_band.float().cpu().numpy()
    rows = dump_rows(out.shape[2], out.shape[0] * out.shape[1] * out.shape[3] * out.itemsize, DUMP_BUDGET_BYTES // world)
    if rows is not None:
        out = np.ascontiguousarray(out[:, :, rows])
    name = "output.npy" if world == 1 else f"output_rank{rank}.npy"
    np.save(os.path.join(directory, name), out)


def effective_cores() -> int:
    """CPU cores this process may actually use: affinity mask capped by the cgroup CPU quota
    (the GPU box exposes 256 logical CPUs but limits the container to a quota of 16)."""
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except Exception:
        pass
    return cores


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import diinn_oracle as orc
    return orc


def cpu_baseline(sd, feat_cpu, size, wl_name):
    """Reference-faithful CPU decode (oracle/) timed on this host: a bounded sample of the benchmarked
    workload on all usable cores (the headline `value`), plus the SURVEY §8 d7 / BASELINE.md §3 legs:
    one thread, config 1 (48^2 -> 96^2) and 128^2 -> 512^2."""
    orc = _oracle()
    import diinn_amd.synth as synth
    cores = effective_cores()
    hu, wu = size
    h = feat_cpu.shape[2]

    def band(rows, threads):
        torch.set_num_threads(threads)
        idx, _ = orc.axis_tables(h, hu, orc.uses_small_output_kernel(hu, wu))
        a1 = min(int(idx[rows - 1]) + 2, h)
        crop = feat_cpu[:, :, :a1].contiguous()
        t0 = time.perf_counter()
        orc.decode_reference_form(sd, crop, size, 30000, row_range=(0, rows), feat_row0=0, full_h=h)
        return time.perf_counter() - t0

    def sized(threads, budget_s):
        probe_rows = min(hu, 16)
        t_probe = band(probe_rows, threads)
        rows = int(min(hu, max(probe_rows, budget_s / max(t_probe, 1e-3) * probe_rows)))
        if rows > 64:
            rows -= rows % 64
        t = band(rows, threads)
        return rows, t

    rows_n, t_n = sized(cores, 8.0)
    rows_1, t_1 = sized(1, 3.0)

    def whole(hw, out, threads, reps):
        torch.set_num_threads(threads)
        f = synth.encoder_features(123, 1, hw, hw)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            orc.decode_reference_form(sd, f, (out, out), 30000)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    t_c1_n = whole(48, 96, cores, 7)
    t_c1_1 = whole(48, 96, 1, 3)
    t_128 = whole(128, 512, cores, 2)
    torch.set_num_threads(cores)
    return {
        "value": round(rows_n * wu / t_n / 1e6, 5),
        "unit": "Mpixels/s",
        "cores": cores,
        "kind": "port",
        "cpu_model": cpu_model(),
        "sample": f"{wl_name} workload, HR rows 0..{rows_n} of {hu} ({rows_n * wu} px), reference-form torch-CPU oracle "
                  f"(unfold -> nearest-exact -> 9 conv1x1 + cat + sin, bsize=30000), {cores} threads, {t_n:.2f} s",
        "one_thread": {"value": round(rows_1 * wu / t_1 / 1e6, 5), "cores": 1,
                       "sample": f"same workload, HR rows 0..{rows_1}, {t_1:.2f} s"},
        "c1_48x48_x2": {"value": round(96 * 96 / t_c1_n / 1e6, 5), "cores": cores, "ms": round(t_c1_n * 1e3, 2),
                        "one_thread_value": round(96 * 96 / t_c1_1 / 1e6, 5), "one_thread_ms": round(t_c1_1 * 1e3, 2),
                        "sample": "whole image, bsize=30000, median of 7 (n threads) / 3 (1 thread)"},
        "lr128_x4": {"value": round(512 * 512 / t_128 / 1e6, 5), "cores": cores, "ms": round(t_128 * 1e3, 1),
                     "sample": "128x128 -> 512x512 whole image, bsize=30000, median of 2"},
    }


def load_traffic():
    """HBM bytes per decode-kernel launch from the committed rocprofv3 --pmc summary (or None)."""
    p = os.path.join(ROOT, "profiles", "decode_kernel_traffic.json")
    try:
        with open(p) as f:
            return json.load(f).get("hbm_bytes_per_launch")
    except Exception:
        return None


def measure_traffic(args, kernel_prefix="void decode_kernel<", timeout_s=90):
    """HBM bytes per launch of the dominant kernel, MEASURED by this run: two `rocprofv3 --pmc` passes of this very script
    (FETCH_SIZE and WRITE_SIZE do not fit one pass; MI355X_MICROARCH.md, HBM / rocprofv3 sections) in child processes --
    `rocprofv3 --kernel-trace --pmc <counter> -- python3 bench.py --steps 3 --warmup 1` with every extra leg off --
    averaged over that kernel's dispatches and corrected as the guide prescribes for gfx950: FETCH_SIZE tallies a wide
    streaming read at half its bytes, so bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024 (the counters are in KB).
    Returns (bytes or None, description).  Never raises: a box without a working profiler yields (None, why)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    vals = {}
    tmp = tempfile.mkdtemp(prefix="diinn_pmc_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            cmd = [prof, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "--",
                   sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                   "--workload", args.workload, "--compute", args.compute, "--no-cpu-baseline",
                   "--no-check", "--no-target", "--no-split", "--no-side-legs", "--no-traffic"]
            if args.sin != "default":
                cmd += ["--sin", args.sin]
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
            env["TMPDIR"] = "/tmp"
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {counter} exited {r.returncode}: {r.stderr[-300:]}"
            got = []
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row["Kernel_Name"].startswith(kernel_prefix) and row["Counter_Name"] == counter:
                        got.append(float(row["Counter_Value"]))
            if not got:
                return None, f"rocprofv3 --pmc {counter}: no rows for {kernel_prefix!r}"
            vals[counter] = (sum(got) / len(got), len(got))
    except Exception as e:                                        # timeout, unreadable csv, ...
        return None, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fetch, nf = vals["FETCH_SIZE"]
    write, nw = vals["WRITE_SIZE"]
    return int((2.0 * fetch + write) * 1024), (
        f"measured by this run: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `bench.py --steps 3 --warmup 1` "
        f"in child processes, mean over {nf} / {nw} dispatches of {kernel_prefix}...>: FETCH_SIZE {fetch:.0f} KB, "
        f"WRITE_SIZE {write:.0f} KB; bytes = (2 x FETCH_SIZE + WRITE_SIZE) x 1024 (gfx950 counts wide reads at 1/2)")


def check_band_rows(sd, feat_win_cpu, feat_row0, full_h, size, out_band_cpu, band_y0, rows_list, compute):
    """max error of the timed output against the oracle on the given HR row ranges (inside this rank's band)."""
    orc = _oracle()
    tol_rel, floor_one = CHECK_TOL[compute]
    worst, ok = 0.0, True
    for (y0, y1) in rows_list:
        ref = orc.decode_reference_form(sd, feat_win_cpu, size, 30000, row_range=(y0, y1),
                                        feat_row0=feat_row0, full_h=full_h).numpy()
        got = out_band_cpu[:, :, y0 - band_y0:y1 - band_y0].numpy()
        err = float(abs(got - ref).max())
        scale = float(abs(ref).max())
        tol = tol_rel * (max(1.0, scale) if floor_one else scale)
        worst = max(worst, err)
        ok = ok and (err <= tol) and bool((got == got).all())
    return worst, ok


def pct(xs, q):
    xs = sorted(xs)
    if not xs:
        return None
    i = min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))
    return xs[i]


class Job:
    """Process-wide state of one bench.py run: ranks, device, collective backend, library handles."""

    def __init__(self, args):
        self.args = args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:                                # (the bare form, WORLD_SIZE unset, never gets here:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={self.world}: the launcher's rank count and --gpus "   # _self_launch_if_bare)
                             f"must agree (one rank per GPU)")
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a ROCm GPU: the DIINN decode path has no CPU implementation")
        if os.environ.get("DIINN_BENCH_ONE_DEVICE") == "1":   # test hook: every rank on cuda:0 (with --backend gloo this
            local_rank = 0                                    # runs every N>1 branch on a one-GPU box)
        torch.cuda.set_device(local_rank)
        self.dev = torch.device("cuda", local_rank)
        self.use_dist = self.world > 1 or "RANK" in os.environ     # launched by torch.distributed.run
        self.gloo = args.backend == "gloo"
        if self.use_dist:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29500")
            # an explicit collective timeout: a rank that never shows up (or a hung hand-off) ends the job with an error
            # inside the driver's budget instead of the 10-30 minute defaults; the watchdog in main() is the backstop
            tmo = datetime.timedelta(seconds=args.dist_timeout)
            if self.gloo:
                dist.init_process_group("gloo", rank=self.rank, world_size=self.world, timeout=tmo)
            else:
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.dev, timeout=tmo)
            dist.barrier()           # first RCCL call is a plain collective on every rank
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))   # as launched (the one-device test hook computes on cuda:0 all the same)

        import diinn_amd._native as N
        import diinn_amd.decoder as D
        import diinn_amd.sharded as S
        import diinn_amd.synth as synth
        self.N, self.D, self.S, self.synth = N, D, S, synth
        self.lib = N.load()
        self.sin_mode = {"accurate": N.SIN_ACCURATE, "hw": N.SIN_HW, "hw_reduced": N.SIN_HW_REDUCED,
                         "default": N.SIN_DEFAULT}[args.sin]
        self.sin_name = {N.SIN_ACCURATE: "accurate", N.SIN_HW: "hw", N.SIN_HW_REDUCED: "hw_reduced"}[self.sin_mode]
        self.comp = N.COMPUTE[args.compute]
        self.sd = synth.decoder_state_dict(123)
        self.packed = D.pack_state_dict(self.sd).to(self.dev)

    def census(self):
        """Who took part: one record per rank -- rank, local rank, the device it computed on (index,
        name, UUID, PCI bus id), the collective backend, how many of the node's other GPUs it can reach peer-to-peer (xGMI) --
        gathered on every rank through the backend itself, plus the world size the backend reports and the number of DISTINCT
        devices.  From the JSON line alone a reader can tell whether RCCL saw N ranks on N devices."""
        # (the local part never raises: every rank must reach the collective below; a query the runtime lacks reads "unknown")
        me = {"rank": self.rank, "local_rank": self.local_rank, "device": self.dev.index, "name": "unknown", "device_uuid": "",
              "pci_bus_id": "", "backend": "none", "visible_devices": -1, "xgmi_peers": -1, "host": socket.gethostname(),
              "pid": os.getpid()}
        try:
            me["backend"] = dist.get_backend() if self.use_dist else "none"
            prop = torch.cuda.get_device_properties(self.dev)
            me["name"] = prop.name
            me["device_uuid"] = str(getattr(prop, "uuid", ""))
            me["pci_bus_id"] = "%04x:%02x:%02x" % (getattr(prop, "pci_domain_id", 0), getattr(prop, "pci_bus_id", 0),
                                                   getattr(prop, "pci_device_id", 0))
            ndev = me["visible_devices"] = torch.cuda.device_count()
            me["xgmi_peers"] = sum(bool(torch.cuda.can_device_access_peer(self.dev.index, other))
                                   for other in range(ndev) if other != self.dev.index)
        except Exception as e:                                    # noqa: BLE001
            me["census_error"] = f"{type(e).__name__}: {e}"
        ranks = [me]
        if self.use_dist:
            try:
                got = [None] * self.world
                dist.all_gather_object(got, me)
                ranks = got
            except Exception as e:                                # noqa: BLE001  (the headline must not depend on this record)
                me["census_error"] = f"all_gather_object: {type(e).__name__}: {e}"
        ids = {(r["host"], r["device_uuid"] or r["pci_bus_id"] or str(r["device"])) for r in ranks}
        return {"ranks": ranks, "rccl_world": (dist.get_world_size() if self.use_dist else 1),
                "backend": me["backend"], "distinct_devices": len(ids)}

    # collectives of the harness itself (timing / verdict exchange): host tensors on gloo, device tensors on RCCL
    def _t(self, vals):
        return torch.tensor(vals, dtype=torch.float64, device="cpu" if self.gloo else self.dev)

    def reduce_max(self, vals):
        if not self.use_dist:
            return [float(v) for v in vals]
        t = self._t(vals)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(v) for v in t.cpu()]

    def bcast_from0(self, t64):
        """float64 device tensor, published by rank 0."""
        if not self.use_dist:
            return t64
        if self.gloo:
            h = t64.cpu()
            dist.broadcast(h, src=0)
            return h.to(t64.device)
        dist.broadcast(t64, src=0)
        return t64

    def barrier(self):
        torch.cuda.synchronize()
        if self.use_dist:
            dist.barrier()
        torch.cuda.synchronize()


def run_workload(job, name, scaling, steps, warmup, solo=False, check=True, gather=False, compute=None):
    """Time ``steps`` steps of one workload.  ``solo``: rank 0 decodes the whole image alone (the same-run one-GPU
    reference of a strong-scaling leg) while the other ranks wait at the barriers.  Returns a dict on every rank
    (timings are this rank's, ``elapsed`` the max over ranks)."""
    args, N, S, lib, dev = job.args, job.N, job.S, job.lib, job.dev
    compute = compute or args.compute                      # (the split-bf16 side leg overrides the run's mode)
    comp = N.COMPUTE[compute]
    world = 1 if solo else job.world
    rank = job.rank
    idle = solo and rank != 0
    (h1, w1), (hu1, wu1), wl_label = WORKLOADS[name]
    mult = world if scaling == "weak" else 1
    H, W, HU, WU = h1 * mult, w1, hu1 * mult, wu1
    shape = (1, 64, H, W)
    res = {"H": H, "W": W, "HU": HU, "WU": WU, "label": wl_label, "world": world}
    if idle:
        job.barrier()
        job.barrier()
        res["elapsed"] = job.reduce_max([0.0])[0]
        if check:
            job.reduce_max([0.0, 0.0])
        return res

    # rank 0 holds the encoder output (synthetic, seeded); every other rank only ever sees the rows handed to it
    feat = None
    if rank == 0:
        gen = torch.Generator(device=dev)
        gen.manual_seed(123)
        feat = torch.randn(shape, device=dev, generator=gen)
    dec = S.BandDecoder(shape, (HU, WU), job.packed, src=0, mode=args.dist_mode, sin_mode=job.sin_mode,
                        compute=compute, solo=solo)
    bd = dec.band
    if bd.empty:
        raise SystemExit("more ranks than HR rows")
    stream = torch.cuda.current_stream().cuda_stream
    mk = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    # Per-kernel HIP events are recorded on every EV_EVERY-th step of the timed loop (>= 3 steps of it): an event
    # record costs ~4 us of stream time (tools/event_overhead.py: 4 per step add 15 us to the 117 us c1 step and 18 us to
    # the 6.12 ms c2 step), so sampling keeps the instrument out of the number it sits in; with one rank the hand-off
    # is empty and its two stamps are one.
    ev_every = max(1, min(4, steps // 3)) if steps < 32 else steps // 8      # long runs (c1: 200 steps): 8 sampled steps
    ev = {i: (mk(), mk(), mk(), mk()) for i in range(0, steps, ev_every)}
    res["event_steps"] = len(ev)
    packed = job.packed
    one_rank = world == 1

    def step(i=None):
        i = i if i in ev else None
        if i is not None and not one_rank:
            ev[i][0].record()
        win, row0 = dec.handoff(feat)            # rank 0: sends started on the side stream, not awaited
        if i is not None:
            ev[i][1].record()
        N.check(lib.diinn_precompute_P_win(C.c_void_p(stream), C.c_void_p(win.data_ptr()), row0, win.shape[2],
                                           C.c_void_p(packed.data_ptr()), C.c_void_p(dec.p_win.data_ptr()),
                                           bd.r0, bd.r1 - bd.r0, 1, H, W, bd.r0, bd.r1, comp), "diinn_precompute_P_win")
        if i is not None:
            ev[i][2].record()
        N.check(lib.diinn_decode_band_win(C.c_void_p(stream), C.c_void_p(dec.p_win.data_ptr()), bd.r0, bd.r1 - bd.r0,
                                          C.c_void_p(packed.data_ptr()), C.c_void_p(dec.out_band.data_ptr()),
                                          bd.y0, bd.y1 - bd.y0, 1, H, W, HU, WU, bd.y0, bd.y1, job.sin_mode, comp),
                "diinn_decode_band_win")
        if i is not None:
            ev[i][3].record()
        dec.complete()                           # order the stream behind the sends (after the kernels are queued)
        return win, row0

    for _ in range(warmup):
        win, row0 = step()
    job.barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        win, row0 = step(i)
    job.barrier()
    elapsed = time.perf_counter() - t0
    res["elapsed"] = job.reduce_max([elapsed])[0] if not solo else elapsed
    if solo:
        job.reduce_max([elapsed])                # pairs with the idle ranks' call
    evs = [ev[i] for i in sorted(ev)]
    res.update(
        bd=bd, dec=dec,
        step_ms=[e[1 if one_rank else 0].elapsed_time(e[3]) for e in evs],
        hand_ms=[0.0 if one_rank else e[0].elapsed_time(e[1]) for e in evs],
        p_ms=[e[1].elapsed_time(e[2]) for e in evs],
        k_ms_all=[e[2].elapsed_time(e[3]) for e in evs],
    )

    # ---- the output that was timed, against the oracle (outside the timed region)
    if check:
        # transport check: rank 0 publishes (sum, sum of squares) of every rank's window in float64; each rank
        # recomputes them on what it received (the same reduction on the same values on the same kind of device)
        handoff_ok = True
        if job.use_dist and world > 1:
            sums = torch.zeros((world, 2), device=dev, dtype=torch.float64)
            if rank == 0:
                for r, b2 in enumerate(dec.bands):
                    if not b2.empty:
                        w64 = feat[:, :, b2.a0:b2.a1].double()
                        sums[r, 0], sums[r, 1] = w64.sum(), (w64 * w64).sum()
            sums = job.bcast_from0(sums)
            lo = bd.a0 - row0
            mine = win[:, :, lo:lo + bd.a1 - bd.a0].double()
            got = torch.stack([mine.sum(), (mine * mine).sum()])
            handoff_ok = bool(torch.allclose(got, sums[rank], rtol=1e-12, atol=0.0))
        nrows = min(4, bd.y1 - bd.y0)
        mid = (bd.y0 + bd.y1) // 2
        starts = sorted({bd.y0, max(bd.y0, min(bd.y1 - nrows, mid)), bd.y1 - nrows})
        rows_list = [(s, s + nrows) for s in starts]
        lo = bd.a0 - row0
        win_cpu = win[:, :, lo:lo + bd.a1 - bd.a0].cpu()       # the rows this rank actually decoded from
        out_cpu = dec.out_band.cpu()
        torch.set_num_threads(max(1, effective_cores() // job.world))   # every rank checks at once on the one host
        err, ok = check_band_rows(job.sd, win_cpu, bd.a0, H, (HU, WU), out_cpu, bd.y0, rows_list, compute)
        ok = ok and handoff_ok
        err, bad = job.reduce_max([err, 0.0 if ok else 1.0])
        tol = CHECK_TOL[compute]
        res["checked"] = {"rows": [list(r) for r in rows_list], "rows_of": "rank 0's band; every rank checks its own",
                          "max_err": err, "tol": f"{tol[0]:g} x max(1,|ref|)" if tol[1] else f"{tol[0]:g} x max|ref|",
                          "handoff_exact": handoff_ok, "ok": bad == 0.0}

    if gather:
        full = torch.empty((1, 3, HU, WU), device=dev) if rank == 0 else None
        for _ in range(2):
            dec.gather(dec.out_band, dst=0, out=full)
        job.barrier()
        tg = time.perf_counter()
        for _ in range(5):
            dec.gather(dec.out_band, dst=0, out=full)
        job.barrier()
        res["gather_ms"] = (time.perf_counter() - tg) / 5 * 1e3
        if check and rank == 0:                  # the assembled image holds rank 0's own band and the last band intact
            last = dec.bands[-1]
            res["gather_ok"] = bool(torch.equal(full[:, :, bd.y0:bd.y1], dec.out_band)) and \
                bool(torch.isfinite(full[:, :, last.y0:last.y1]).all())
    res["feat"] = feat
    return res


STRONG_LEGS = {2: ["tgt", "c3"], 4: ["tgt", "c3"], 8: ["tgt", "c4"]}      # north_star target; BASELINE c3 (2, 4), c4 (8)


def strong_legs(job):
    """For N > 1: ONE image split into N row bands against the same image decoded by rank 0 alone in the same run
    (the north_star's ">= 6x tile-parallel scaling at 8 GPUs" is a strong-scaling claim; the headline is weak)."""
    args = job.args
    names = args.strong_legs.split(",") if args.strong_legs else STRONG_LEGS.get(job.world, ["tgt"])
    legs = []
    for name in [n for n in names if n]:
        steps = args.strong_steps
        many = run_workload(job, name, "strong", steps, 1, check=not args.no_check, gather=args.gather)
        hand = job.reduce_max([statistics.median(many["hand_ms"])])[0]       # the slowest receiver
        kern = job.reduce_max([statistics.median(many["step_ms"])])[0]
        checked = many.get("checked")
        g_ok = many.get("gather_ok")
        ms_n = many["elapsed"] / steps * 1e3
        del many
        torch.cuda.empty_cache()
        one = run_workload(job, name, "strong", steps, 1, solo=True, check=False)
        ms_1 = job.reduce_max([one["elapsed"] / steps * 1e3])[0]
        del one
        torch.cuda.empty_cache()
        (h, w), (hu, wu), label = WORKLOADS[name]
        leg = {"workload": name, "what": label, "n_gpus": job.world, "steps": steps,
               "ms_1gpu": round(ms_1, 4), "ms_Ngpu": round(ms_n, 4),
               "speedup": round(ms_1 / ms_n, 3), "efficiency": round(ms_1 / ms_n / job.world, 4),
               "handoff_ms": round(hand, 4), "slowest_band_ms": round(kern, 4),
               "mpix_s_Ngpu": round(hu * wu / ms_n / 1e3, 2),
               "note": "ms = wall per step between barriers, max over ranks; handoff_ms = slowest rank's median "
                       "HIP-event time in the hand-off (receivers wait for their rows; rank 0 overlaps its sends)"}
        if checked is not None:
            leg["checked_ok"] = checked["ok"]
            leg["max_err"] = checked["max_err"]
        if g_ok is not None:
            leg["gather_ok"] = g_ok
        legs.append(leg)
    return legs


# Driver-timed side legs of the default N = 1 run: the other single-GPU BASELINE configs, a few
# steps each, so that their numbers are measured by the same run that produces the headline -- never part of `value`.
SIDE_LEGS = [("c5", "f32", 2, 1), ("c5", "bf16_full", 5, 2), ("c5", "bf16", 5, 2), ("c1", "f32", 200, 20)]   # c5 bf16 = SURVEY d4's 2e-3 variant


def decode_kernel_name(job, b, hu, wu, y0, y1, compute):
    """The decode kernel the library launches for these rows (its own choice: diinn_decode_kernel_info), for labels."""
    N = job.N
    info = (C.c_int * 4)()
    N.check(job.lib.diinn_decode_kernel_info(b, hu, wu, y0, y1, 0, wu, N.COMPUTE[compute], info), "diinn_decode_kernel_info")
    if info[0] == 1:
        return "decode_kernel"
    if info[0] == 3:
        return "decode_coop16_kernel"
    return "decode_bf16x3 kernel" if compute == "bf16x3" else "decode_bf16 kernel"


def side_leg(job, name, compute, steps, warmup, check=True):
    t = run_workload(job, name, "strong", steps, warmup, check=check, compute=compute)
    (h, w), (hu, wu), label = WORKLOADS[name]
    t_k = sum(t["k_ms_all"]) / len(t["k_ms_all"])
    p_ms = sum(t["p_ms"]) / len(t["p_ms"])
    bf = compute != "f32"
    peak = PEAK_BF16_MFMA_TFLOPS if bf else PEAK_F32_MFMA_TFLOPS
    ach = FLOP_DECODE_PER_PX * hu * wu / (t_k * 1e-3) / 1e12
    leg = {"workload": label, "name": name, "compute": compute, "steps": steps, "warmup": warmup,
           "ms_per_step": round(t["elapsed"] / steps * 1e3, 4),
           "mpix_s": round(hu * wu * steps / t["elapsed"] / 1e6, 2),
           "kernel_ms": round(t_k, 4), "kernel_ms_min": round(min(t["k_ms_all"]), 4), "p_kernel_ms": round(p_ms, 4),
           "achieved": round(ach, 2), "peak": peak, "frac": round(ach / peak, 4),
           "kernel": decode_kernel_name(job, 1, hu, wu, 0, hu, compute),
           "of": f"decode kernel, HIP events on {t['event_steps']} of the {steps} steps; frac = 789,504 FLOP/px x pixels / "
                 f"kernel time / the dense {'bf16' if bf else 'fp32'} MFMA peak"}
    if "checked" in t:
        leg["checked"] = t["checked"]
    del t
    torch.cuda.empty_cache()
    return leg


def whole_model_leg(device, steps=5, warmup=2, lr=256, scale=4):
    """Informational, never part of `value`: the callers' path -- DIINN.forward (reference: diinn.py:9-30: RDN encoder, then the
    implicit decoder) on a random lr x lr image (256 x4: BASELINE config 2's geometry with the encoder the reference pairs it
    with; 48 x2 / x4: the reference's own timing protocol, runtime_test.py:13,31-33,59-62, and its training crops), random-init
    weights: whole forward, encoder alone, decoder alone, in ms (torch events on the current stream)."""
    import diinn_amd.modules as M
    torch.manual_seed(0)
    net = M.DIINN(mode=3, init_q=False).to(device).eval()
    x = torch.rand(1, 3, lr, lr, device=device)
    size = (lr * scale, lr * scale)

    def t_ms(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize(device)
        return e0.elapsed_time(e1) / steps

    with torch.no_grad():
        feat = net.encoder(x)
        fwd = t_ms(lambda: net(x, size))
        enc = t_ms(lambda: net.encoder(x))
        dec = t_ms(lambda: net.decoder(feat, size, 30000))
        out = net(x, size)
    import diinn_amd._native as N
    leg = {"workload": f"DIINN.forward: RDN encoder + implicit decoder, {lr}x{lr} LR x{scale} ({size[0]}x{size[1]}), B = 1, random-init weights",
           "steps": steps, "warmup": warmup, "forward_ms": round(fwd, 3), "encoder_ms": round(enc, 3), "decoder_ms": round(dec, 3),
           "finite": bool(torch.isfinite(out).all()),
           "handoff_gave_up": int(M.RDN.handoff_status(clear=False)),     # the F(4x4) split hand-off's sticky status (0: never gave up)
           "encoder_3x3_layers": ("Winograd F(4x4,3x3)" if net.encoder.hip_winograd4 and N.load().diinn_rdn_wino4_applies(1, lr, lr)
                                  else "Winograd F(2x2,3x3)" if lr * lr >= 8192
                                  else "direct, strips of 16 pixels x 16 outputs (conv_t16_kernel)" if N.load().diinn_conv_t16_applies(1, lr, lr)
                                  else "direct, split-K"),
           "note": "parity of this path: tests/test_modules.py (reference DIINN fixture), tests/test_encoder_trunk.py (the real reference's encoder)"}
    del net, x, feat, out
    torch.cuda.empty_cache()
    return leg


def training_leg(device, steps=5, warmup=2, b=16, lr=48, scale=4):
    """Informational, never part of `value`: one training step of the DECODER (reference: sr_module.py:127-137 calls
    forward with grad and bsize=None) at the reference's training geometry (configs/default.yaml: batch 16, 48 x 48 LR patches, scales
    2-4): forward with saved planes + backward, every kernel the library's own (no library convolution or GEMM), in ms."""
    import diinn_amd.decoder as D
    import diinn_amd.synth as synth
    dec = D.ImplicitDecoder(mode=3, init_q=False)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state_dict(123).items()})
    dec = dec.to(device).train()
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(device).requires_grad_(True)
    hu = wu = lr * scale
    r = torch.randn(b, 3, hu, wu, device=device)

    def step():
        dec.zero_grad(set_to_none=True)
        feat.grad = None
        (dec(feat, [hu, wu]) * r).sum().backward()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(device)
    ms = (time.perf_counter() - t0) / steps * 1e3
    ok = bool(torch.isfinite(feat.grad).all()) and all(bool(torch.isfinite(p.grad).all()) for p in dec.parameters())
    leg = {"workload": f"decoder training step (forward with saved planes + backward), B = {b}, {lr}x{lr} LR x{scale} ({hu}x{wu}): "
                       f"{b * hu * wu} HR pixels", "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 3),
           "mpix_s": round(b * hu * wu / ms / 1e3, 2), "finite_grads": ok,
           "note": "gradient parity: tests/test_training.py (fixtures from the real reference's autograd); kernel times: profiles/r06_train_kernel_stats.csv"}
    del dec, feat, r
    torch.cuda.empty_cache()
    return leg


def main():
    args = parse()
    # stdout carries exactly ONE line, the JSON result: the collective libraries print banners to stdout when they
    # initialise ("RCCL version : ...", "[Gloo] Rank 0 is connected to ..."), so file descriptor 1 points at stderr
    # until the line is written
    sys.stdout.flush()
    result_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    if args.watchdog > 0:
        def _expired():
            sys.stderr.write(f"bench.py: rank {os.environ.get('RANK', '0')} still running after {args.watchdog} s "
                             f"(hung collective or hand-off?): exiting with code 124\n")
            sys.stderr.flush()
            os._exit(124)
        wd = threading.Timer(args.watchdog, _expired)
        wd.daemon = True
        wd.start()
    job = Job(args)
    world, rank = job.world, job.rank
    N = job.N
    census = job.census()
    full = args.full                                       # everything beyond the headline runs only with --full

    r = run_workload(job, args.workload, args.scaling, args.steps, args.warmup, check=full and not args.no_check,
                     gather=args.gather)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, r["dec"].out_band, rank, world)
    elapsed, bd = r["elapsed"], r["bd"]
    H, W, HU, WU, wl_label = r["H"], r["W"], r["HU"], r["WU"], r["label"]
    (h1, w1), (hu1, wu1), _ = WORKLOADS[args.workload]
    step_ms, hand_ms, p_ms, k_ms_all = r["step_ms"], r["hand_ms"], r["p_ms"], r["k_ms_all"]
    event_steps = r["event_steps"]
    checked, gather_ms, gather_ok = r.get("checked"), r.get("gather_ms"), r.get("gather_ok")
    feat_cpu = r["feat"].cpu() if (full and rank == 0 and world == 1 and not args.no_cpu_baseline) else None
    hand_max = job.reduce_max([statistics.median(hand_ms)])[0]
    # which form of the hoisted conv the library ran for this launch (diinn_p_launch_info: env overrides included)
    p_algo = C.c_int(0)
    N.check(job.lib.diinn_p_launch_info(1, H, W, bd.r0, bd.r1, job.comp, C.byref(p_algo)), "diinn_p_launch_info")
    p_wino = p_algo.value == N.P_ALGO_WINOGRAD
    p_x3 = p_algo.value == N.P_ALGO_DIRECT_BF16X3
    del r
    torch.cuda.empty_cache()

    split = None
    if full and world == 1 and args.workload == "c2" and args.compute == "f32" and not args.no_split:
        # the same workload in the optional split-bf16 mode (DIINN_COMPUTE_BF16X3: bf16 MFMAs, three products per term,
        # held to the fp32 bound by the same post-run check): reported beside the fp32 line, never as `value`
        t = run_workload(job, "c2", "weak", args.steps, args.warmup, compute="bf16x3")
        t_k = sum(t["k_ms_all"]) / len(t["k_ms_all"])
        split = {"compute": "bf16x3", "mpix_s": round(t["HU"] * t["WU"] * args.steps / t["elapsed"] / 1e6, 2),
                 "ms_per_step": round(t["elapsed"] / args.steps * 1e3, 4), "kernel": "decode_bf16x3 kernel",
                 "kernel_ms": round(t_k, 4), "p_kernel_ms": round(sum(t["p_ms"]) / len(t["p_ms"]), 4),
                 "issued_bf16_tflops": round((3 * 786_432.0 + 3_072.0) * t["HU"] * t["WU"] / (t_k * 1e-3) / 1e12, 1),
                 "checked": t.get("checked"),
                 "note": "hi/lo bf16 operands, hi*hi + hi*lo + lo*hi with fp32 accumulation; same workload, same "
                         "1e-4 x max(1,|ref|) check against the oracle as the fp32 line"}
        del t
        torch.cuda.empty_cache()
    strong = None
    if full and world > 1 and not args.no_strong:
        strong = strong_legs(job)
    target = None
    if full and world == 1 and args.workload == "c2" and args.compute == "f32" and not args.no_target:
        # the north_star's target shape (1024^2 -> 4096^2 on one GPU) timed by the same run: 1 warm-up + 2 steps
        t = run_workload(job, "tgt", "strong", 2, 1, check=False)
        t_k = sum(t["k_ms_all"]) / len(t["k_ms_all"])
        t_ach = FLOP_DECODE_PER_PX * 4096 * 4096 / (t_k * 1e-3) / 1e12
        target = {"workload": WORKLOADS["tgt"][2], "steps": 2, "ms": round(t["elapsed"] / 2 * 1e3, 3),
                  "mpix_s": round(4096 * 4096 / (t["elapsed"] / 2) / 1e6, 2), "kernel_ms": round(t_k, 3),
                  "achieved": round(t_ach, 2), "frac": round(t_ach / PEAK_F32_MFMA_TFLOPS, 4),
                  "p_kernel_ms": round(sum(t["p_ms"]) / len(t["p_ms"]), 3),
                  "note": "decode_kernel's share of the fp32 MFMA peak at the target shape; parity at this size: "
                          "tests/test_gpu_configs.py::test_target_1024_x4"}
        del t
        torch.cuda.empty_cache()

    side = whole = None
    if full and world == 1 and args.workload == "c2" and args.compute == "f32" and not args.no_side_legs:
        side = [side_leg(job, n, c, st, wu_, check=not args.no_check) for (n, c, st, wu_) in SIDE_LEGS]
        try:
            whole = whole_model_leg(job.dev)
            # the reference's own timing protocol (runtime_test.py: a 48 x 48 crop) at x2 and x4: encoder-bound
            whole["small_inputs"] = [whole_model_leg(job.dev, steps=20, warmup=5, lr=48, scale=2),
                                     whole_model_leg(job.dev, steps=20, warmup=5, lr=48, scale=4)]
            whole["training_step"] = training_leg(job.dev)
        except Exception as e:                                   # informational leg: report, do not lose the line
            whole = {"error": f"{type(e).__name__}: {e}"}

    k_ms = sum(k_ms_all) / max(len(k_ms_all), 1)
    px_launch = (bd.y1 - bd.y0) * WU
    achieved = FLOP_DECODE_PER_PX * px_launch / (k_ms * 1e-3) / 1e12
    p_mean = sum(p_ms) / max(len(p_ms), 1)
    p_tflops = FLOP_P_PER_CELL * (bd.r1 - bd.r0) * W / (p_mean * 1e-3) / 1e12

    if rank == 0:
        total_px = HU * WU
        ms_per_step = elapsed / args.steps * 1e3
        bf = args.compute != "f32"
        peak = PEAK_BF16_MFMA_TFLOPS if bf else PEAK_F32_MFMA_TFLOPS
        p_peak = PEAK_BF16_MFMA_TFLOPS if (args.compute == "bf16_full" or p_x3) else PEAK_F32_MFMA_TFLOPS
        if args.scaling == "weak":
            wl = (f"{wl_label} per GPU, {HU}x{WU} HR total ({world} row band(s) of {hu1}x{WU}), B=1, mode=3")
        else:
            wl = (f"{wl_label}, split into {world} HR row band(s) of ~{HU // world}x{WU}, B=1, mode=3")
        traffic, traffic_source = None, None
        if not bf and args.workload == "c2" and world == 1:
            why = "--no-traffic"
            if not full:
                why = "measured only with --full"
            elif "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
                why = "this run is itself being profiled"
            elif not args.no_traffic:
                traffic, traffic_source = measure_traffic(args)
                why = traffic_source
            if traffic is None:                                  # no profiler on this box: the committed measurement, labelled
                traffic = load_traffic()
                traffic_source = ("profiles/decode_kernel_traffic.json: separate rocprofv3 --pmc passes of this command, "
                                  f"committed; NOT measured in this run ({why})")
        res = {
            "metric": METRIC[args.workload],
            "value": round(total_px * args.steps / elapsed / 1e6, 3),
            "unit": "Mpixels/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": args.compute,
            "data": "synthetic",
            "config": {
                "workload": wl, "name": args.workload,
                "lr": [H, W], "hr": [HU, WU], "sin": job.sin_name,
                "parallelism": f"hr-row-bands x{world}" + (f" ({args.dist_mode} feature hand-off, {args.backend})"
                                                           if world > 1 else ""),
                "step": "feature hand-off (N>1; rank 0's sends overlap its own band) + precompute_P + decode_kernel, "
                        "band-sized buffers",
            },
            "step_ms": {"min": round(min(step_ms), 4), "median": round(statistics.median(step_ms), 4),
                        "p90": round(pct(step_ms, 0.9), 4), "mean_wall": round(ms_per_step, 4),
                        "handoff_median": round(statistics.median(hand_ms), 4),
                        "handoff_median_slowest_rank": round(hand_max, 4),
                        "of": f"rank 0, HIP events on {event_steps} of the {args.steps} timed steps"},
            "roofline": {
                "bound": "mfma",
                "kernel": decode_kernel_name(job, 1, HU, WU, bd.y0, bd.y1, args.compute),
                "achieved": round(achieved, 3),
                "peak": peak,
                "unit": "TFLOP/s",
                "frac": round(achieved / peak, 4),
                "kernel_ms": round(k_ms, 4),
                "kernel_ms_min": round(min(k_ms_all), 4),
                "kernel_launches_timed": event_steps,
                "flop_per_launch": FLOP_DECODE_PER_PX * px_launch,
                "traffic": traffic,
                "traffic_source": traffic_source,
                "p_kernel": {"ms": round(p_mean, 4), "ms_min": round(min(p_ms), 4),
                             "algorithm": "winograd F(2x2,3x3)" if p_wino else ("direct, split bf16" if p_x3 else "direct"),
                             "frac": round(p_tflops * (3.0 if p_x3 else 1.0) / (2.25 if p_wino else 1.0) / p_peak, 4),
                             "direct_equiv_tflops": round(p_tflops, 2),
                             "direct_equiv_frac": round(p_tflops / p_peak, 4),
                             "note": "frac = MFMA work actually issued / peak (the roofline fraction); direct_equiv_* "
                                     "count the 1,179,648 direct-convolution FLOP per cell the Winograd form avoids "
                                     "2.25x of -- a speed figure, not a utilisation"},
            },
        }
        if args.compute == "bf16x3":
            # split bf16 issues three bf16 MFMAs per fp32-equivalent one in layers 1..3 (786,432 of the 789,504 FLOP)
            issued = (3 * 786_432.0 + 3_072.0) * px_launch / (k_ms * 1e-3) / 1e12
            res["roofline"]["issued_tflops"] = round(issued, 2)
            res["roofline"]["issued_frac"] = round(issued / peak, 4)
            res["roofline"]["note"] = ("achieved counts the algorithm's 789,504 FLOP per pixel once; the kernel issues "
                                       "3 bf16 MFMAs per product (hi*hi + hi*lo + lo*hi): issued_* is the matrix-core load")
        if bf and args.compute != "bf16x3":
            # second roof for the bf16 path: the vector L1 (64 B/clk/CU).  The cooperative kernel
            # moves, per 128-pixel block, 768 KiB of weights (each wave its own slice, no reuse between waves), 4 slices
            # of up to 24 staged P rows of 1 KiB, and ~8 KiB of tables through it; VALU / LDS / wait shares from the PMC
            # passes are in profiles/r02_pmc_summary.txt.
            l1_bytes_px = (768 * 1024 + 4 * 24 * 1024 + 8 * 1024) / 128.0
            l1_peak = 64.0 * 256 * 2.4e9 / 1e12                      # TB/s at 2.4 GHz
            l1_ach = l1_bytes_px * px_launch / (k_ms * 1e-3) / 1e12
            res["roofline_l1"] = {"bound": "vector L1", "bytes_per_pixel": round(l1_bytes_px), "achieved": round(l1_ach, 2),
                                  "peak": round(l1_peak, 1), "unit": "TB/s", "frac": round(l1_ach / l1_peak, 4),
                                  "note": "weight refills arrive in bursts (one per layer, all 8 waves at once): the "
                                          "bound is the burst, not the average"}
        # who ran: N > 1 must show N ranks on N distinct devices on the real backend ("nccl" = RCCL); the one-device test
        # transport shows N ranks on 1 device
        res["rccl_world"] = census["rccl_world"]
        res["backend"] = census["backend"]
        res["distinct_devices"] = census["distinct_devices"]
        res["ranks"] = census["ranks"]
        if checked is not None:
            res["checked"] = checked
        if gather_ms is not None:
            res["gather_ms"] = round(gather_ms, 4)
        if gather_ok is not None:
            res["gather_ok"] = gather_ok
        if split is not None:
            res["split_bf16"] = split
        if target is not None:
            res["target_shape"] = target
        if side is not None:
            res["side_legs"] = side
        if whole is not None:
            res["whole_model"] = whole
        if strong is not None:
            res["strong"] = strong
        if feat_cpu is not None:
            res["cpu_baseline"] = cpu_baseline(job.sd, feat_cpu, (HU, WU), args.workload)
        print(json.dumps(res), file=result_out, flush=True)
    if job.use_dist:
        dist.barrier()
        dist.destroy_process_group()
    # every check the run made decides its exit status: the headline, the split-bf16 and side legs, the strong legs,
    # the gather
    def _bad(c):
        return c is not None and not c["ok"]
    failed = _bad(checked) or (gather_ok is False) or \
        _bad((split or {}).get("checked")) or any(_bad(leg.get("checked")) for leg in (side or [])) or \
        any(not leg.get("checked_ok", True) or leg.get("gather_ok") is False for leg in (strong or []))
    if failed:
        raise SystemExit(f"bench.py: timed output failed a check: headline {checked} gather_ok {gather_ok} "
                         f"split {(split or {}).get('checked')} side {[l.get('checked') for l in (side or [])]} strong {strong}")


if __name__ == "__main__":
    main()
