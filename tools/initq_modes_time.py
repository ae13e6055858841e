"""Decoder ``init_q=True`` with modes 1, 2 and 4 (``ImplicitDecoder.hip_initq_modes``): time of ``ImplicitDecoder.forward`` on the
HIP path against the reference's op sequence in PyTorch-ROCm eager on the same device, at c2 (256 x 256 x4, B = 1) and at B = 16
of 48 x 48 x4; beside it mode 3 + init_q, whose kernels this path leaves alone, on this build and on another build of the
library (the parent commit's), and the two forms of the planes launch.

    python tools/initq_modes_time.py                              # modes 1, 2, 4: HIP and eager, alternating run by run
    python tools/initq_modes_time.py --planes                     # one chunk: the 512-row planes launch (mode 1) against the 1280-row one
    python tools/initq_modes_time.py --mode3                      # mode 3 + init_q on this build (the parent commit's figure: its own
                                                                  # ``tools/initq_time.py --hip-only --warmup 5`` from a checkout of it,
                                                                  # the two commands alternating in one session)

Device events around each run, after warm-ups (5 warm-ups, 20 runs).  The eager comparison is the reference's sequence written
out with public PyTorch ops (diinn.py:94-147,149-173) over column strips of ``bsize = 30000`` pixels; its result is checked
against the HIP result before anything is timed.  Mode 4: the reference pads every strip, so its strips do not give the
whole-image result the HIP path reproduces; the check runs the sequence on the whole image, the timing on strips.

``F_alg`` per HR pixel: mode 2 2,264,064 FLOP (planes 1,474,560; chain 393,216; the synthesis halves of layers 1-3 393,216; head
and sine inputs 3,072), mode 1 1,379,328 (planes 589,824), mode 4 2,276,352 (mode 3's 2,264,064 with 27 head rows in place of
3); over the fp32 matrix peak of 157.3 TFLOP/s."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import diinn_amd._native as N  # noqa: E402
import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

CONFIGS = [("c2  256x256 x4  B=1", 1, 256, 256, 1024, 1024), ("48x48 x4  B=16", 16, 48, 48, 192, 192)]
F_STEP = {1: 1_379_328, 2: 2_264_064, 3: 2_264_064, 4: 2_276_352}
PEAK = 157.3e12


def eager_forward(wt, x, size, mode, bsize=30000):
    """The reference's eager sequence with init_q (fp32, inference); ``bsize=None``: the whole image at once."""
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
            if mode == 1:
                k = torch.relu(conv(k, f"K.{i}.0"))
            else:
                k = torch.relu(conv(torch.cat([k if mode == 2 else q, xs], 1), f"K.{i}.0"))
            q = k * torch.sin(conv(q, f"Q.{i}.0"))
        if mode == 4:
            return F.conv2d(F.pad(q, (1, 1, 1, 1), mode="reflect"), wt["last_layer.weight"], wt["last_layer.bias"])
        return conv(q, "last_layer")

    if bsize is None:
        return step(xu, syn)
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


def line(tag, ms, npix=None, flops=None):
    med = statistics.median(ms)
    tail = "" if npix is None else f"  F_alg / t / peak = {npix * flops / (med * 1e-3) / PEAK:.3f}"
    return f"{tag:52s} median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs){tail}"


def decoder(mode, dev, sin_mode):
    sd = synth.decoder_state_dict(123, mode=mode, init_q=True)
    kw = {} if sin_mode is None else {"sin_mode": sin_mode}
    dec = D.ImplicitDecoder(mode=mode, init_q=True, hip_initq_modes=mode != 3, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec.to(dev).eval()


def time_modes(a, dev):
    for mode in a.modes:
        dec = decoder(mode, dev, a.sin_mode)
        wt = {k: v.detach() for k, v in dec.state_dict().items()}
        for name, b, h, w, hu, wu in CONFIGS:
            feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
            npix = b * hu * wu

            def hip():
                with torch.no_grad():
                    return dec(feat, (hu, wu), 30000)

            def eager():
                with torch.no_grad():
                    return eager_forward(wt, feat, (hu, wu), mode, 30000)

            fns = [("HIP  ImplicitDecoder.forward", hip)] + ([] if a.hip_only else [("eager reference sequence, bsize 30000", eager)])
            for _ in range(a.warmup):
                outs = [fn() for _, fn in fns]
            torch.cuda.synchronize()
            if not a.hip_only:
                with torch.no_grad():
                    ref = eager_forward(wt, feat, (hu, wu), mode, None) if mode == 4 else outs[1]
                err = float((outs[0] - ref).abs().max())
                tol = 1e-4 * max(1.0, float(ref.abs().max()))
                print(f"mode {mode}  {name}: max|hip - eager| = {err:.3e} (contract {tol:.1e}); chunks of "
                      f"{D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES)} rows")
                assert err <= tol
                del ref
            del outs
            ms = {tag: [] for tag, _ in fns}
            for _ in range(a.runs):                                      # alternating, run by run
                for tag, fn in fns:
                    ms[tag].append(run_ms(fn))
            for tag, _ in fns:
                print(line(f"mode {mode}  {name}  {tag}", ms[tag], npix, F_STEP[mode]), flush=True)
            if not a.hip_only:
                h_, e_ = statistics.median(ms[fns[0][0]]), statistics.median(ms[fns[1][0]])
                print(f"mode {mode}  {name}: HIP / eager = {h_ / e_:.3f}  ({'faster' if h_ < e_ else 'NOT faster'})", flush=True)


def time_mode3(a, dev):
    dec = decoder(3, dev, a.sin_mode)
    for name, b, h, w, hu, wu in CONFIGS:
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)

        def hip():
            with torch.no_grad():
                return dec(feat, (hu, wu), 30000)

        for _ in range(a.warmup):
            hip()
        torch.cuda.synchronize()
        print(line(f"mode 3  {name}  HIP  ImplicitDecoder.forward", [run_ms(hip) for _ in range(a.runs)], b * hu * wu, F_STEP[3]), flush=True)


def time_planes(a, dev):
    """One chunk of the c2 decode (48 rows x 1024 columns): the two forms of the planes launch and the two chains, alternating."""
    lib = N.load()
    b, h, w, hu, wu = CONFIGS[0][1:]
    rows = D.initq_chunk_rows(b, wu, D.ImplicitDecoder.INITQ_CHUNK_BYTES)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    pix = torch.empty(b * rows * wu * 1280, device=dev)
    sin_mode = N.SIN_DEFAULT if a.sin_mode is None else a.sin_mode
    ptr = lambda t: C.c_void_p(t.data_ptr())
    images = {}
    for mode in (1, 2):
        sd = synth.decoder_state_dict(123, mode=mode, init_q=True)
        images[mode] = (D.pack_state_dict(D.initq_body_state_dict(sd), mode=mode).to(dev), D.pack_initq(sd).to(dev))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def planes(mode, fn):
        packed, iq = images[mode]
        return lambda: N.check(fn(stream, ptr(feat), ptr(packed), ptr(iq), ptr(pix), b, h, w, hu, wu, 0, rows, sin_mode), "planes")

    def chain(mode):
        return lambda: N.check(lib.diinn_pixel_chain(stream, ptr(pix), ptr(images[mode][0]), b, wu, rows, int(mode == 1)), "chain")

    fns = [("initq_planes_kernel<SIN | INITQ_ROWS512> (mode 1)", planes(1, lib.diinn_initq_planes_m1), 589_824),
           ("initq_planes_kernel<SIN> (mode 2)", planes(2, lib.diinn_initq_planes), 1_474_560),
           ("pixel_chain_kernel<BK_SEEDS> (mode 1)", chain(1), 393_216),
           ("pixel_chain_kernel (mode 2)", chain(2), 393_216)]
    for _ in range(a.warmup):
        for _, fn, _ in fns:
            fn()
    torch.cuda.synchronize()
    ms = {tag: [] for tag, _, _ in fns}
    for _ in range(a.runs):
        for tag, fn, _ in fns:
            ms[tag].append(run_ms(fn))
    print(f"one chunk of c2: {rows} rows x {wu} columns = {rows * wu} pixels")
    for tag, _, fl in fns:
        print(line(tag, ms[tag], b * rows * wu, fl), flush=True)
    m1, m2 = statistics.median(ms[fns[0][0]]), statistics.median(ms[fns[1][0]])
    print(f"planes launch, mode 1 / mode 2 = {m1 / m2:.3f}  (FLOP count: 0.400)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 2, 4], choices=[1, 2, 4])
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--planes", action="store_true")
    ap.add_argument("--mode3", action="store_true")
    ap.add_argument("--sin-mode", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    print(f"device {torch.cuda.get_device_name(0)}; sin_mode {N.SIN_DEFAULT if a.sin_mode is None else a.sin_mode}; "
          f"chunk cap {D.ImplicitDecoder.INITQ_CHUNK_BYTES >> 20} MiB", flush=True)
    if a.mode3:
        time_mode3(a, dev)
    elif a.planes:
        time_planes(a, dev)
    else:
        time_modes(a, dev)


if __name__ == "__main__":
    main()
