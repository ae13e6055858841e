"""Decoder modes 1, 2 and 4 (``init_q=False``): time of ``ImplicitDecoder.forward`` in split-bf16 arithmetic
(``hip_modes_split_bf16`` with ``compute="bf16x3"``: the Q-only / the tap form of ``decode_bf16x3_kernel``) against the fp32 forward
of the same mode on the same build, at c2 (256 x 256 x4, B = 1) and at B = 16 of 48 x 48 x4.

    python tools/modes_x3_time.py                # modes 1, 2, 4; the two arithmetics alternating run by run in one process
    python tools/modes_x3_time.py --mode3        # mode 3 as well (fp32 against "bf16x3": kernels this opt-in does not touch)
    python tools/modes_x3_time.py --x3-only      # the split-bf16 paths alone (the form to put under rocprofv3 --kernel-trace --stats)

Device events around each run, after warm-ups; median, min and max of --runs runs.  The two results of a mode are compared
before anything is timed (the contract, 1e-4 x max(1, max|fp32|)).  A mode counts as faster only when its slowest split-bf16 run
beats its fastest fp32 run."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

CONFIGS = [("c2  256x256 x4  B=1", 1, 256, 256, 1024, 1024), ("48x48 x4  B=16", 16, 48, 48, 192, 192)]


def run_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def line(tag, ms):
    return f"{tag:52s} median {statistics.median(ms):9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--x3-only", action="store_true")
    ap.add_argument("--mode3", action="store_true")
    ap.add_argument("--sin-mode", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    kw = {} if a.sin_mode is None else {"sin_mode": a.sin_mode}
    print(f"device {torch.cuda.get_device_name(0)}; sin_mode {D.ImplicitDecoder(**kw).sin_mode}")
    for mode in ([1, 2, 3, 4] if a.mode3 else [1, 2, 4]):
        sd = synth.decoder_state_dict(123, mode=mode)

        def module(**more):
            dec = D.ImplicitDecoder(mode=mode, init_q=False, **kw, **more)
            dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            return dec.to(dev).eval()

        f32, x3 = module(), module(compute="bf16x3", hip_modes_split_bf16=True)
        for name, b, h, w, hu, wu in CONFIGS:
            feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)

            def run_x3():
                with torch.no_grad():
                    return x3(feat, (hu, wu), 30000)

            def run_f32():
                with torch.no_grad():
                    return f32(feat, (hu, wu), 30000)

            fns = ([] if a.x3_only else [("fp32  ImplicitDecoder.forward", run_f32)]) + [("split bf16  ImplicitDecoder.forward", run_x3)]
            for _ in range(a.warmup):
                outs = [fn() for _, fn in fns]
            torch.cuda.synchronize()
            if not a.x3_only:
                err = float((outs[0] - outs[1]).abs().max())
                tol = 1e-4 * max(1.0, float(outs[0].abs().max()))
                print(f"mode {mode}  {name}: max|split bf16 - fp32| = {err:.3e} (contract {tol:.1e})")
                assert err <= tol
            del outs
            ms = {tag: [] for tag, _ in fns}
            for _ in range(a.runs):                                      # alternating, run by run
                for tag, fn in fns:
                    ms[tag].append(run_ms(fn))
            for tag, _ in fns:
                print(line(f"mode {mode}  {name}  {tag}", ms[tag]), flush=True)
            if not a.x3_only:
                f_, x_ = ms[fns[0][0]], ms[fns[1][0]]
                fm, xm = statistics.median(f_), statistics.median(x_)
                clear = max(x_) < min(f_)
                print(f"mode {mode}  {name}: split bf16 / fp32 = {xm / fm:.3f} = {fm / xm:.2f}x  "
                      f"({'faster by more than the spread' if clear else 'NOT clearly faster'}: "
                      f"fp32 {min(f_):.3f}..{max(f_):.3f}, split bf16 {min(x_):.3f}..{max(x_):.3f})", flush=True)


if __name__ == "__main__":
    main()
