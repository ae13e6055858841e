"""Decoder ``init_q=True`` with modes 1, 2 and 4 in split-bf16 arithmetic (``ImplicitDecoder.hip_initq_modes`` +
``hip_initq_modes_split_bf16``, ``compute="bf16x3"``): time of ``ImplicitDecoder.forward`` in fp32 and in split bf16 on the SAME build
and the SAME module, alternating run by run, at c2 (256 x 256 x4, B = 1) and at B = 16 of 48 x 48 x4.  (Mode 3 + init_q in both
arithmetics, whose kernels this path leaves alone: tools/initq_x3_time.py, from this build and from a checkout of the parent commit,
the two commands alternating in one session.)

    python tools/initq_modes_x3_time.py                       # modes 1, 2, 4: fp32 and split bf16, alternating
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/initq_modes_x3_time.py --runs 3 --warmup 1 --configs 0
                                                              # per-kernel times of the three launches (a run of its own: tracing
                                                              # slows the host, so its forward times are not the ones to quote)

Device events around each forward, after warm-ups of both arithmetics (5 warm-ups, 20 runs).  The split result is checked against
the fp32 result (the contract, 1e-4 x max(1, max|fp32|)) before anything is timed.  Acceptance, per mode and geometry: the SLOWEST
split-bf16 run is faster than the FASTEST fp32 run of the same process; the tool says so and exits non-zero otherwise.

``F_alg`` per HR pixel as in tools/initq_modes_time.py (mode 2 2,264,064 FLOP: planes 1,474,560; chain 393,216; synthesis
393,216; head and sine inputs 3,072; mode 1 1,379,328; mode 4 2,276,352).  The split arithmetic runs three bf16 MFMA products per
term: the figure printed is F_alg / t, what the user gets, not the matrix cores' rate."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import diinn_amd._native as N  # noqa: E402
import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

CONFIGS = [("c2  256x256 x4  B=1", 1, 256, 256, 1024, 1024), ("48x48 x4  B=16", 16, 48, 48, 192, 192)]
F_STEP = {1: 1_379_328, 2: 2_264_064, 4: 2_276_352}


def run_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def line(tag, ms, npix, flops):
    med = statistics.median(ms)
    return (f"{tag:44s} median {med:8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  ({len(ms)} runs)  "
            f"F_alg / t = {npix * flops / (med * 1e-3) / 1e12:6.1f} TFLOP/s")


def decoder(mode, dev, sin_mode):
    sd = synth.decoder_state_dict(123, mode=mode, init_q=True)
    kw = {} if sin_mode is None else {"sin_mode": sin_mode}
    dec = D.ImplicitDecoder(mode=mode, init_q=True, hip_initq_modes=True, hip_initq_modes_split_bf16=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec.to(dev).eval()


def time_modes(a, dev, modes):
    ok = True
    for mode in modes:
        dec = decoder(mode, dev, a.sin_mode)
        for name, b, h, w, hu, wu in [CONFIGS[i] for i in a.configs]:
            feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
            npix = b * hu * wu

            def forward(compute):
                def fn():
                    dec.compute = compute
                    with torch.no_grad():
                        return dec(feat, (hu, wu), 30000)
                return fn

            fns = [("fp32", forward("f32")), ("split bf16", forward("bf16x3"))]
            for _ in range(a.warmup):
                outs = [fn() for _, fn in fns]
            torch.cuda.synchronize()
            err = float((outs[0] - outs[1]).abs().max())
            tol = 1e-4 * max(1.0, float(outs[0].abs().max()))
            print(f"mode {mode}  {name}: max|split - fp32| = {err:.3e} (contract {tol:.1e}); chunks of "
                  f"{D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES)} rows")
            assert err <= tol and not torch.equal(outs[0], outs[1])
            del outs
            ms = {tag: [] for tag, _ in fns}
            for _ in range(a.runs):                                      # alternating, run by run
                for tag, fn in fns:
                    ms[tag].append(run_ms(fn))
            for tag, _ in fns:
                print(line(f"mode {mode}  {name}  {tag}", ms[tag], npix, F_STEP[mode]), flush=True)
            f_, s_ = ms["fp32"], ms["split bf16"]
            faster = max(s_) < min(f_)
            print(f"mode {mode}  {name}: split / fp32 = {statistics.median(s_) / statistics.median(f_):.3f} (medians); slowest split "
                  f"{max(s_):.3f} ms {'<' if faster else '>='} fastest fp32 {min(f_):.3f} ms: {'faster' if faster else 'NOT faster'}", flush=True)
            ok = ok and faster
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 2, 4], choices=[1, 2, 4])
    ap.add_argument("--configs", type=int, nargs="+", default=[0, 1], choices=[0, 1])
    ap.add_argument("--sin-mode", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    print(f"device {torch.cuda.get_device_name(0)}; sin_mode {N.SIN_DEFAULT if a.sin_mode is None else a.sin_mode}; "
          f"chunk cap {D.ImplicitDecoder.INITQ_CHUNK_BYTES >> 20} MiB", flush=True)
    if not time_modes(a, dev, a.modes):
        sys.exit("a split-bf16 run was not faster than every fp32 run")


if __name__ == "__main__":
    main()
