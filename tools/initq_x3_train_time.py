#!/usr/bin/env python3
"""Decoder ``init_q=True`` (mode 3) training step in split-bf16 arithmetic against the fp32 step, on one GPU.

  fp32   : initq_training.DecodeInitqFunction (initq_planes_kernel<RAD>, decode_kernel<INITQ, SAVE>; bwd_layer_kernel x 3,
           initq_bwd_kernel; the plane GEMMs, row products, cell sum and fold)
  split  : initq_split_training.DecodeInitqSplitFunction (initq_planes_x3_kernel<RAD>, decode_bf16x3_kernel<INITQ | SAVE>;
           bwd_layer_x3_kernel x 3, initq_bwd_x3_kernel; the same plane GEMMs, row products, cell sum and fold)

The two steps alternate in one process, 2 warm-ups and medians of ``--runs`` (20) single steps each, with min and max.  Also
printed: the forward under grad of each, the exchanged kernels side by side (events around the C ABI calls on the step's own
buffers), initq_bwd_x3_kernel's share of a third of the bf16 matrix peak (three MFMA products per useful one: 2 x 640 x 1280 FLOP per
pixel count once), the device packers, peak memory of a step of each path, and every gradient's distance from float64 with PINNED
gates for the split path at ``--dist-batch`` images (2).  No time is asserted anywhere.

usage: initq_x3_train_time.py [B] [LR] [SCALE] [--runs=N] [--dist-batch=N] [--only-split] [--default-off]
       (default 16 48 4: the reference's training patch; c2 is 1 256 4)
       --only-split:  5 split steps and nothing else, for a kernel trace
       --default-off: the paths the switch leaves alone, timed with events (medians of --runs): the fp32 init_q step, mode 3's split
                      step and init_q split inference -- to be run alternately on this build and on the parent commit's
                      (DIINN_HIP_LIB selects the library)
"""
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diinn_amd._native as N  # noqa: E402
import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.initq_training as IT  # noqa: E402
import diinn_amd.split_training as ST  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402
import diinn_amd.training as T  # noqa: E402

PEAK_F32, PEAK_X3 = 157.3e12, 2500e12 / 3


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return f"{median(xs):8.2f} ms   (min {min(xs):.2f}, max {max(xs):.2f}; {len(xs)} runs)"


def timed(fn, runs):
    for _ in range(2):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return median([e0.elapsed_time(e1) for e0, e1 in ev])


def default_off(b, lr, hu, wu, dev, runs):
    """The three default-off neighbours of the new route: none of them runs a kernel or an image this path adds."""
    sdq = synth.decoder_state_dict(123, 1.0, mode=3, init_q=True)
    sd3 = synth.decoder_state_dict(123, 1.0, mode=3)
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)

    def decoder(sd, **kw):
        dec = D.ImplicitDecoder(mode=3, **kw)
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        return dec.to(dev).train()

    decq = decoder(sdq, init_q=True, hip_autograd=True)
    dec3 = decoder(sd3, compute="bf16x3", hip_autograd_split_bf16=True)
    deci = decoder(sdq, init_q=True, compute="bf16x3", hip_initq_split_bf16=True).eval()

    def step(dec):
        def fn():
            dec.zero_grad(set_to_none=True)
            feat.grad = None
            (dec(feat, (hu, wu)) * r).sum().backward()
        return fn

    def infer():
        with torch.no_grad():
            deci(feat.detach(), (hu, wu))

    fns = [("fp32 init_q training step", step(decq)), ("mode 3 split training step", step(dec3)), ("init_q split inference", infer)]
    for _, fn in fns:
        fn()
        fn()
    ts = {tag: [] for tag, _ in fns}
    for _ in range(runs):
        for tag, fn in fns:
            ts[tag].append(once(fn))
    print(f"  library: {N.LIB_PATH}")
    for tag, _ in fns:
        print(f"  {tag:30s} {spread(ts[tag])}")


def main():
    argv = [a for a in sys.argv if not a.startswith("--")]
    runs = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--runs=")), 20)
    dist_b = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--dist-batch=")), 2)
    b = int(argv[1]) if len(argv) > 1 else 16
    lr = int(argv[2]) if len(argv) > 2 else 48
    sc = int(argv[3]) if len(argv) > 3 else 4
    hu = wu = lr * sc
    dev = torch.device("cuda:0")
    n = b * hu * wu
    print(f"init_q decoder (mode 3), fp32 and split bf16  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels; device {torch.cuda.get_device_name(0)}")
    if "--default-off" in sys.argv:
        default_off(b, lr, hu, wu, dev, runs)
        return
    import diinn_amd.initq_split_training as IS
    sd = synth.decoder_state_dict(123, 1.0, mode=3, init_q=True)
    named = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sd.items()}
    params = [named[k] for k in IT.INITQ_PARAM_NAMES]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)

    def zero():
        feat.grad = None
        for p in params:
            p.grad = None

    def step_of(function):
        def fn():
            zero()
            (function.apply(feat, hu, wu, N.SIN_DEFAULT, *params) * r).sum().backward()
        return fn

    f32_step, x3_step = step_of(IT.DecodeInitqFunction), step_of(IS.DecodeInitqSplitFunction)
    if "--only-split" in sys.argv:
        for _ in range(5):
            x3_step()
        torch.cuda.synchronize()
        return

    def f32_fwd():
        IT.DecodeInitqFunction.apply(feat, hu, wu, N.SIN_DEFAULT, *params)

    def x3_fwd():
        IS.DecodeInitqSplitFunction.apply(feat, hu, wu, N.SIN_DEFAULT, *params)

    fns = [("step fwd+bwd, fp32", f32_step), ("step fwd+bwd, split bf16", x3_step), ("forward under grad, fp32", f32_fwd),
           ("forward under grad, split bf16", x3_fwd)]
    for _, fn in fns:
        fn()
        fn()
    peaks = {}
    for tag, fn in fns[:2]:
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks[tag] = torch.cuda.max_memory_allocated() / 2**30
    ts = {tag: [] for tag, _ in fns}
    for _ in range(runs):
        for tag, fn in fns:
            ts[tag].append(once(fn))
    for tag, _ in fns:
        print(f"  {tag:32s} {spread(ts[tag])}")
    print(f"  fp32 / split = {median(ts[fns[0][0]]) / median(ts[fns[1][0]]):.2f}; slowest split step {max(ts[fns[1][0]]):.2f} ms, "
          f"fastest fp32 step {min(ts[fns[0][0]]):.2f} ms")
    print(f"  peak memory of a step: fp32 {peaks[fns[0][0]]:.2f} GiB, split bf16 {peaks[fns[1][0]]:.2f} GiB")

    # the split backward against the float64 formula sheet GIVEN the planes its own forward saved, at a smaller batch: no gate luck
    db = min(dist_b, b)
    ps = [p.detach() for p in params]
    f_s, r_s = feat.detach()[:db].contiguous(), r[:db].contiguous()
    _, acts_s, packed_s, image_s, split_s, iqs_s = IS.train_forward_initq_split(f_s, ps, hu, wu, N.SIN_DEFAULT)
    d_f, d_p = IT.backward_fused_initq(r_s, f_s, acts_s, packed_s, image_s, (hu, wu), split=split_s, initq_split=iqs_s)
    plain = T.untile_planes(acts_s, db * hu * wu).reshape(4, 2, 256, -1).double()
    w_f, w_p = IT.backward_from_saved_initq(r_s.double(), f_s.double(), plain, [p.double() for p in ps], (hu, wu))
    dist = [(float((a.double() - e).abs().max()) / float(e.abs().max()), name) for name, a, e in zip(["feat"] + IT.INITQ_PARAM_NAMES, [d_f] + d_p, [w_f] + w_p)]
    print(f"  largest max|g_split - float64 given the saved planes| / max|float64| at B={db} ({db * hu * wu} pixels): {max(dist)[0]:.2e} ({max(dist)[1]})")
    del acts_s, plain, d_f, d_p, w_f, w_p

    # the exchanged kernels side by side, on buffers of the step's shapes
    lib = N.load()
    feat_c = feat.detach().contiguous()
    out, acts, packed, image, split, iqs = IS.train_forward_initq_split(feat_c, ps, hu, wu, N.SIN_DEFAULT)
    t = (n + 31) // 32
    gp = r.permute(1, 0, 2, 3).reshape(3, n).contiguous()
    g = torch.empty((4, t, 512, 32), device=dev)
    q = torch.empty((4, t, 256, 32), device=dev)
    u_t, da_t = torch.empty((t, 576, 32), device=dev), torch.empty((t, 576, 32), device=dev)
    xp_t, e_t = torch.empty((t, 640, 32), device=dev), torch.empty((t, 640, 32), device=dev)
    pix = torch.empty(lib.diinn_initq_pix_bytes(b, wu, hu) // 4, device=dev)
    out2, acts2 = torch.empty_like(out), torch.empty_like(acts)
    split2, iqs2 = torch.empty_like(split), torch.empty_like(iqs)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    geom = (b, lr, lr, hu, wu)
    ks = {
        "diinn_decode_initq_train_fwd    (fp32)": lambda: N.check(lib.diinn_decode_initq_train_fwd(stream, ptr(feat_c), ptr(packed), ptr(image), ptr(pix), ptr(out2), ptr(acts2), *geom, N.SIN_DEFAULT), "fwd"),
        "diinn_decode_initq_train_fwd_x3 (split)": lambda: N.check(lib.diinn_decode_initq_train_fwd_x3(stream, ptr(feat_c), ptr(packed), ptr(image), ptr(split), ptr(iqs), ptr(pix), ptr(out2), ptr(acts2), *geom, N.SIN_DEFAULT), "fwd x3"),
        "diinn_backward_data    (fp32, 3 kernels)": lambda: N.check(lib.diinn_backward_data(stream, ptr(gp), ptr(acts), ptr(packed), ptr(g), ptr(q), n), "bwd"),
        "diinn_backward_data_x3 (split, 3 kernels)": lambda: N.check(lib.diinn_backward_data_x3(stream, ptr(gp), ptr(acts), ptr(packed), ptr(split), ptr(g), ptr(q), n), "bwd x3"),
        "diinn_initq_backward    (initq_bwd_kernel)": lambda: N.check(lib.diinn_initq_backward(stream, ptr(feat_c), ptr(g), ptr(image), ptr(u_t), ptr(da_t), ptr(xp_t), ptr(e_t), *geom), "initq bwd"),
        "diinn_initq_backward_x3 (initq_bwd_x3_kernel)": lambda: N.check(lib.diinn_initq_backward_x3(stream, ptr(feat_c), ptr(g), ptr(image), ptr(iqs), ptr(u_t), ptr(da_t), ptr(xp_t), ptr(e_t), *geom), "initq bwd x3"),
        "diinn_pack_split_train + diinn_pack_initq_split_train": lambda: (N.check(lib.diinn_pack_split_train(stream, ptr(packed), ptr(split2)), "pack"),
                                                                          N.check(lib.diinn_pack_initq_split_train(stream, ptr(packed), ptr(image), ptr(iqs2)), "pack iqs")),
    }
    res = {tag: timed(fn, runs) for tag, fn in ks.items()}
    f_init, f_useful = 2.0 * 640 * 1280 * n, 2.0 * 576 * 1280 * n
    for tag, ms in res.items():
        extra = ""
        if "initq_bwd_kernel" in tag:
            extra = f"   issued {f_init / ms / 1e9:.1f} TFLOP/s = {f_init / ms * 1e3 / PEAK_F32:.3f} of the fp32 matrix peak"
        if "initq_bwd_x3_kernel" in tag:
            extra = (f"   issued {f_init / ms / 1e9:.1f} TFLOP/s = {f_init / ms * 1e3 / PEAK_X3:.3f} of a third of the bf16 matrix peak "
                     f"(useful {f_useful / ms * 1e3 / PEAK_X3:.3f}); moves {n * (5120 + 2 * 2304 + 9728) / ms / 1e6:.0f} GB/s of planes")
        print(f"  {tag:54s} {ms:8.3f} ms{extra}")


if __name__ == "__main__":
    main()
