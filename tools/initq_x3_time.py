"""Decoder ``init_q=True`` (mode 3): time of ``ImplicitDecoder.forward`` in split-bf16 arithmetic (``hip_initq_split_bf16`` with
``compute="bf16x3"``: ``initq_planes_x3_kernel`` + ``decode_bf16x3_kernel<SIN | X3_INITQ>``, row chunks) against the fp32 ``init_q``
forward of the same build (``initq_planes_kernel`` + ``decode_kernel<SIN | DECODE_INITQ>``), at c2 (256 x 256 x4, B = 1) and at
B = 16 of 48 x 48 x4.

    python tools/initq_x3_time.py                # both, alternating run by run in one process: median, min, max of --runs runs
    python tools/initq_x3_time.py --x3-only      # the split-bf16 path alone (the form to put under rocprofv3 --kernel-trace --stats)

Device events around each run, after warm-ups.  The two results are compared before anything is timed (the contract,
1e-4 x max(1, max|fp32|)).  ``F_alg`` = 2,264,064 FLOP per HR pixel for the step (1,474,560 for the two per-pixel GEMMs of the
planes kernel), over the fp32 matrix peak of 157.3 TFLOP/s for the fp32 lines and over a third of the bf16 matrix peak of
2,500 TFLOP/s (nominal) for the split-bf16 lines (three bf16 MFMA products per term)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

CONFIGS = [("c2  256x256 x4  B=1", 1, 256, 256, 1024, 1024), ("48x48 x4  B=16", 16, 48, 48, 192, 192)]
F_STEP, PEAK_F32, PEAK_X3 = 2_264_064, 157.3e12, 2500e12 / 3


def run_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def line(tag, ms, npix, peak):
    med = statistics.median(ms)
    return (f"{tag:44s} median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)  "
            f"F_alg / t / peak = {npix * F_STEP / (med * 1e-3) / peak:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--x3-only", action="store_true")
    ap.add_argument("--sin-mode", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    sd = synth.decoder_state_dict(123, mode=3, init_q=True)
    kw = {} if a.sin_mode is None else {"sin_mode": a.sin_mode}

    def module(**more):
        dec = D.ImplicitDecoder(mode=3, init_q=True, **kw, **more)
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        return dec.to(dev).eval()

    f32, x3 = module(), module(compute="bf16x3", hip_initq_split_bf16=True)
    print(f"device {torch.cuda.get_device_name(0)}; sin_mode {x3.sin_mode}; chunk cap {x3.INITQ_CHUNK_BYTES >> 20} MiB")
    for name, b, h, w, hu, wu in CONFIGS:
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
        npix = b * hu * wu

        def run_x3():
            with torch.no_grad():
                return x3(feat, (hu, wu), 30000)

        def run_f32():
            with torch.no_grad():
                return f32(feat, (hu, wu), 30000)

        fns = ([] if a.x3_only else [("fp32  ImplicitDecoder.forward", run_f32, PEAK_F32)]) + \
            [("split bf16  ImplicitDecoder.forward", run_x3, PEAK_X3)]
        for _ in range(a.warmup):
            outs = [fn() for _, fn, _ in fns]
        torch.cuda.synchronize()
        if not a.x3_only:
            err = float((outs[0] - outs[1]).abs().max())
            tol = 1e-4 * max(1.0, float(outs[0].abs().max()))
            print(f"{name}: max|split bf16 - fp32| = {err:.3e} (contract {tol:.1e}); chunks of "
                  f"{D.initq_chunk_rows(b, wu, x3.INITQ_CHUNK_BYTES)} rows")
            assert err <= tol
        del outs
        ms = {tag: [] for tag, _, _ in fns}
        for _ in range(a.runs):                                      # alternating, run by run
            for tag, fn, _ in fns:
                ms[tag].append(run_ms(fn))
        for tag, _, peak in fns:
            print(line(f"{name}  {tag}", ms[tag], npix, peak), flush=True)
        if not a.x3_only:
            f_, x_ = ms[fns[0][0]], ms[fns[1][0]]
            fm, xm = statistics.median(f_), statistics.median(x_)
            clear = max(x_) < min(f_)
            print(f"{name}: split bf16 / fp32 = {xm / fm:.3f}  ({'faster by more than the spread' if clear else 'NOT clearly faster'}: "
                  f"fp32 {min(f_):.3f}..{max(f_):.3f}, split bf16 {min(x_):.3f}..{max(x_):.3f})", flush=True)


if __name__ == "__main__":
    main()
