"""LIIF decode (``liif_decode_features``: the fp32 hoisted conv + ``liif_kernel``) against the same decode in split-bf16 arithmetic
(``split=``: the same conv + ``liif_x3_kernel``) on the same build, at c2 (256 x 256 x4, B = 1) and at B = 16 of 48 x 48 x4.

    python tools/liif_x3_time.py                 # both geometries; the two arithmetics alternating run by run in one process
    python tools/liif_x3_time.py --f32-only      # the fp32 decode alone (also runs on a build without the split-bf16 entry point)
    python tools/liif_x3_time.py --x3-only       # the split-bf16 decode alone (the form to put under rocprofv3 --kernel-trace --stats)

Every geometry is a step of its own: a child process under ``timeout``, and the first step that fails ends the run.  Device events
around each run, after warm-ups; median, min and max of --runs runs.  The two results are compared before anything is timed (the
contract, 1e-4 x max(1, max|fp32|)).  Split bf16 counts as faster only when its slowest run beats the fastest fp32 run."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("c2  256x256 x4  B=1", 1, 256, 256, 1024, 1024), ("48x48 x4  B=16", 16, 48, 48, 192, 192)]
STEP_SECONDS = 240


def line(tag, ms):
    return f"{tag:52s} median {statistics.median(ms):9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)"


def step(a, index):
    sys.path.insert(0, ROOT)
    import torch
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    import diinn_amd.synth as synth
    assert torch.cuda.is_available(), "needs a ROCm GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    name, b, h, w, hu, wu = CONFIGS[index]
    if index == 0:
        print(f"device {torch.cuda.get_device_name(0)}")
    torch.manual_seed(123)
    net = M.LIIF().eval()
    host = D.pack_liif_state_dict(net.imnet.state_dict(), prefix="")
    packed = host.to(dev)
    split = None if a.f32_only else D.pack_liif_split(host).to(dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    ws = torch.empty(N.load().diinn_workspace_bytes(b, h, w) // 4, device=dev)
    outs = {"fp32": torch.empty((b, 3, hu, wu), device=dev), "x3": torch.empty((b, 3, hu, wu), device=dev)}

    def run_f32():
        D.liif_decode_features(feat, packed, (hu, wu), out=outs["fp32"], workspace=ws)

    def run_x3():
        D.liif_decode_features(feat, packed, (hu, wu), out=outs["x3"], workspace=ws, split=split)

    fns = ([] if a.x3_only else [("fp32  liif_decode_features", run_f32)]) + ([] if a.f32_only else [("split bf16  liif_decode_features", run_x3)])
    for _ in range(a.warmup):
        for _, fn in fns:
            fn()
    torch.cuda.synchronize()
    if len(fns) == 2:
        err = float((outs["fp32"] - outs["x3"]).abs().max())
        tol = 1e-4 * max(1.0, float(outs["fp32"].abs().max()))
        print(f"{name}: max|split bf16 - fp32| = {err:.3e} (contract {tol:.1e})")
        assert err <= tol
    ms = {tag: [] for tag, _ in fns}
    for _ in range(a.runs):                                          # alternating, run by run
        for tag, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[tag].append(e0.elapsed_time(e1))
    for tag, _ in fns:
        print(line(f"{name}  {tag}", ms[tag]), flush=True)
    if len(fns) == 2:
        f_, x_ = ms[fns[0][0]], ms[fns[1][0]]
        fm, xm = statistics.median(f_), statistics.median(x_)
        clear = max(x_) < min(f_)
        print(f"{name}: split bf16 / fp32 = {xm / fm:.3f} = {fm / xm:.2f}x  "
              f"({'faster by more than the spread' if clear else 'NOT clearly faster'}: "
              f"fp32 {min(f_):.3f}..{max(f_):.3f}, split bf16 {min(x_):.3f}..{max(x_):.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--f32-only", action="store_true")
    ap.add_argument("--x3-only", action="store_true")
    ap.add_argument("--step", type=int, default=None, help="(internal) run one geometry in this process")
    a = ap.parse_args()
    if a.step is not None:
        return step(a, a.step)
    for i in range(len(CONFIGS)):                                    # a fresh process per geometry, under its own time limit
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", str(i),
               "--runs", str(a.runs), "--warmup", str(a.warmup)] + (["--f32-only"] if a.f32_only else []) + (["--x3-only"] if a.x3_only else [])
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(f"step {i} ({CONFIGS[i][0]}) ended with status {rc}: stopping")


if __name__ == "__main__":
    main()
