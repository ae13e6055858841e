"""Decoder ``init_q=True`` (mode 3): time of ``ImplicitDecoder.forward`` on the HIP path (``initq_planes_kernel`` +
``decode_kernel<SIN | DECODE_INITQ>``, row chunks) against the reference's op sequence in PyTorch-ROCm eager on the same device, at
c2 (256 x 256 x4, B = 1) and at B = 16 of 48 x 48 x4.

    python tools/initq_time.py                  # both, alternating run by run in one process: median, min, max of --runs runs
    python tools/initq_time.py --hip-only       # the HIP path alone (the form to put under rocprofv3 --kernel-trace --stats)

Device events around each run, after warm-ups.  The eager comparison is the reference's sequence written out with public
PyTorch ops (diinn.py:94-115,132-139,149-173: position encoding, ``first_layer``, the embedding times the up-sampled unfolded
features, the four dual-branch layers as 1x1 convolutions over column strips of ``bsize = 30000`` pixels); its result is checked
against the HIP result before anything is timed.  ``F_alg`` = 2,264,064 FLOP per HR pixel for the step (1,474,560 for the two
per-pixel GEMMs of ``initq_planes_kernel``, 786,432 for layers 1-3, 3,072 for the head and layer-0's sine inputs), over the fp32
matrix peak of 157.3 TFLOP/s."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

CONFIGS = [("c2  256x256 x4  B=1", 1, 256, 256, 1024, 1024), ("48x48 x4  B=16", 16, 48, 48, 192, 192)]
F_STEP, F_PLANES, PEAK = 2_264_064, 1_474_560, 157.3e12


def eager_forward(wt, x, size, bsize=30000):
    """The reference's eager sequence for mode 3 with init_q (fp32, inference)."""
    b, c, h, w = x.shape
    hu, wu = size

    def grid(n):
        return -1 + 1 / n + 2 / n * torch.arange(n, device=x.device).float()

    lo = torch.stack(torch.meshgrid(grid(h), grid(w), indexing="ij"), 0)
    up = torch.stack(torch.meshgrid(grid(hu), grid(wu), indexing="ij"), 0)
    rel = up - F.interpolate(lo[None], size=(hu, wu), mode="nearest-exact")
    rel[:, 0] *= h
    rel[:, 1] *= w
    ratio = x.new_tensor([(h * w) / (hu * wu)]).view(1, -1, 1, 1).expand(b, -1, hu, wu)
    syn = torch.cat([rel.expand(b, -1, hu, wu), ratio], 1)
    xu = F.interpolate(F.unfold(x, 3, padding=1).view(b, c * 9, h, w), size=(hu, wu), mode="nearest-exact")

    def conv(t, name):
        return F.conv2d(t, wt[name + ".weight"], wt[name + ".bias"])

    def step(xs, ss):
        e = torch.sin(conv(ss, "first_layer.0"))
        xs = e * xs
        k = torch.relu(conv(xs, "K.0.0"))
        q = k * torch.sin(conv(e, "Q.0.0"))
        for i in (1, 2, 3):
            k = torch.relu(conv(torch.cat([q, xs], 1), f"K.{i}.0"))
            q = k * torch.sin(conv(q, f"Q.{i}.0"))
        return conv(q, "last_layer")

    preds, ql = [], 0
    while ql < wu:
        qr = min(ql + bsize // hu, wu)
        preds.append(step(xu[:, :, :, ql:qr], syn[:, :, :, ql:qr]))
        ql = qr
    return torch.cat(preds, -1)


def run_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def line(tag, ms, npix, flops):
    med = statistics.median(ms)
    return (f"{tag:44s} median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)  "
            f"F_alg / t / peak = {npix * flops / (med * 1e-3) / PEAK:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--sin-mode", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    sd = synth.decoder_state_dict(123, mode=3, init_q=True)
    kw = {} if a.sin_mode is None else {"sin_mode": a.sin_mode}
    dec = D.ImplicitDecoder(mode=3, init_q=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    dec = dec.to(dev).eval()
    wt = {k: v.detach() for k, v in dec.state_dict().items()}
    print(f"device {torch.cuda.get_device_name(0)}; sin_mode {dec.sin_mode}; chunk cap {dec.INITQ_CHUNK_BYTES >> 20} MiB")
    for name, b, h, w, hu, wu in CONFIGS:
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
        npix = b * hu * wu

        def hip():
            with torch.no_grad():
                return dec(feat, (hu, wu), 30000)

        def eager():
            with torch.no_grad():
                return eager_forward(wt, feat, (hu, wu), 30000)

        fns = [("HIP  ImplicitDecoder.forward", hip)] + ([] if a.hip_only else [("eager reference sequence, bsize 30000", eager)])
        for _ in range(a.warmup):
            outs = [fn() for _, fn in fns]
        torch.cuda.synchronize()
        if not a.hip_only:
            err = float((outs[0] - outs[1]).abs().max())
            tol = 1e-4 * max(1.0, float(outs[1].abs().max()))
            print(f"{name}: max|hip - eager| = {err:.3e} (contract {tol:.1e}); chunks of "
                  f"{D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES)} rows")
            assert err <= tol
        del outs
        ms = {tag: [] for tag, _ in fns}
        for _ in range(a.runs):                                      # alternating, run by run
            for tag, fn in fns:
                ms[tag].append(run_ms(fn))
        for tag, _ in fns:
            print(line(f"{name}  {tag}", ms[tag], npix, F_STEP), flush=True)
        if not a.hip_only:
            h_, e_ = statistics.median(ms[fns[0][0]]), statistics.median(ms[fns[1][0]])
            print(f"{name}: HIP / eager = {h_ / e_:.3f}  ({'faster' if h_ < e_ else 'NOT faster'})", flush=True)


if __name__ == "__main__":
    main()
