#!/usr/bin/env python3
"""LIIF decoder training step (forward + backward) on one GPU: fp32 against split bf16 (``LIIF.hip_autograd_split_bf16``).

  fp32   : liif_training.LIIFFunction        (diinn_liif_train_fwd,    diinn_liif_backward_data)
  split  : liif_split_training.LIIFSplitFunction (diinn_liif_train_fwd_x3, diinn_liif_backward_data_x3); everything else is shared

The two alternate run by run in one process on one build, ``--runs`` (10) single steps each after warm-up; min / median / max are
printed.  Also: the two exchanged entry points alone (events around the C ABI calls on the step's own buffers, alternating as
well), peak memory of a step of each path, and every gradient's distance from float64 with PINNED gates for both paths at
``--dist-batch`` images (2): ``liif_backward_from_saved`` in float64 on the path's own saved planes, upcast.  No time is asserted.

usage: liif_x3_train_time.py [B] [LR] [SCALE] [--runs=N] [--dist-batch=N] [--only-fp32]
       default 16 48 4 (the reference's training patch geometry); c2 is 1 256 4
       --only-fp32: the fp32 step alone (what a build without the split path can run too)
"""
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diinn_amd._native as N  # noqa: E402
import diinn_amd.liif_training as LT  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

SHAPES = {"imnet.layers.0.weight": (256, 580), "imnet.layers.0.bias": (256,),
          **{f"imnet.layers.{i}.weight": (256, 256) for i in (2, 4, 6)}, **{f"imnet.layers.{i}.bias": (256,) for i in (2, 4, 6)},
          "imnet.layers.8.weight": (3, 256), "imnet.layers.8.bias": (3,)}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def mmm(xs):
    return f"{sorted(xs)[len(xs) // 2]:8.3f} ms   (min {min(xs):.3f}, max {max(xs):.3f}; {len(xs)} runs)"


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    argv = [a for a in sys.argv if not a.startswith("--")]
    runs = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--runs=")), 10)
    dist_b = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--dist-batch=")), 2)
    only_fp32 = "--only-fp32" in sys.argv
    b = int(argv[1]) if len(argv) > 1 else 16
    lr = int(argv[2]) if len(argv) > 2 else 48
    sc = int(argv[3]) if len(argv) > 3 else 4
    hu = wu = lr * sc
    dev = torch.device("cuda:0")
    sd = synth.state_dict_for(SHAPES, 123, "liif.")
    params = [torch.from_numpy(sd["imnet." + n]).to(dev).requires_grad_(True) for n in LT.PARAM_NAMES]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)
    n = b * hu * wu
    vn = 4 * n

    def zero():
        feat.grad = None
        for p in params:
            p.grad = None

    def fp32_step():
        zero()
        (LT.LIIFFunction.apply(feat, hu, wu, *params) * r).sum().backward()

    print(f"LIIF decoder  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels, {vn} virtual pixels")
    if only_fp32:
        for _ in range(3):
            fp32_step()
        print(f"  step fwd+bwd, fp32                                {mmm([once(fp32_step) for _ in range(runs)])}")
        return
    import diinn_amd.liif_split_training as LS  # noqa: E402

    def split_step():
        zero()
        (LS.LIIFSplitFunction.apply(feat, hu, wu, *params) * r).sum().backward()

    peak = {}
    for tag, fn in (("fp32", fp32_step), ("split", split_step)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        zero()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[tag] = torch.cuda.max_memory_allocated() / 2**30
    t32, tx3 = [], []
    for _ in range(runs):
        t32.append(once(fp32_step))
        tx3.append(once(split_step))
    print(f"  step fwd+bwd, fp32                                {mmm(t32)}")
    print(f"  step fwd+bwd, split bf16                          {mmm(tx3)}   {median(t32) / median(tx3):.2f}x")
    print(f"  slowest split step {max(tx3):.3f} ms, fastest fp32 step {min(t32):.3f} ms")
    print(f"  peak memory of a step: fp32 {peak['fp32']:.2f} GiB, split bf16 {peak['split']:.2f} GiB")
    zero()

    # the two exchanged entry points alone, on buffers of the step's shapes
    lib = N.load()
    feat_c = feat.detach().contiguous()
    image, split = LT.image_on_device(params), LS.split_on_device(params)
    t = LT.virtual_tiles(n)
    out = torch.empty((b, 3, hu, wu), device=dev)
    acts = torch.empty((4, t, 256, 32), device=dev)
    g = torch.empty((4, t, 256, 32), device=dev)
    wk = torch.empty(lib.diinn_workspace_bytes(b, lr, lr) // 4, device=dev)
    gp = r.permute(1, 0, 2, 3).reshape(3, n).contiguous()
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plane_gb = t * 256 * 32 * 4 / 1e9

    def f32():
        N.check(lib.diinn_liif_train_fwd(stream, ptr(feat_c), ptr(image), ptr(wk), ptr(out), ptr(acts), b, lr, lr, hu, wu), "diinn_liif_train_fwd")

    def fx3():
        N.check(lib.diinn_liif_train_fwd_x3(stream, ptr(feat_c), ptr(image), ptr(split), ptr(wk), ptr(out), ptr(acts), b, lr, lr, hu, wu),
                "diinn_liif_train_fwd_x3")

    def b32():
        N.check(lib.diinn_liif_backward_data(stream, ptr(gp), ptr(acts), ptr(image), ptr(g), b, lr, lr, hu, wu), "diinn_liif_backward_data")

    def bx3():
        N.check(lib.diinn_liif_backward_data_x3(stream, ptr(gp), ptr(acts), ptr(image), ptr(split), ptr(g), b, lr, lr, hu, wu),
                "diinn_liif_backward_data_x3")

    for fn in (f32, fx3, b32, bx3) * 2:
        fn()
    tf32, tfx3, tb32, tbx3 = [], [], [], []
    for _ in range(runs):
        tf32.append(event_ms(f32))
        tfx3.append(event_ms(fx3))
        tb32.append(event_ms(b32))
        tbx3.append(event_ms(bx3))
    flop = 3 * 2.0 * 256 * 256 * vn
    print(f"  diinn_liif_train_fwd (events)                     {mmm(tf32)}   {flop / median(tf32) / 1e9:.1f} TFLOP/s")
    print(f"  diinn_liif_train_fwd_x3 (events)                  {mmm(tfx3)}   {median(tf32) / median(tfx3):.2f}x; writes {4 * plane_gb:.2f} GB of planes"
          f" -> {4 * plane_gb / median(tfx3):.2f} TB/s")
    print(f"  diinn_liif_backward_data (3 kernels)              {mmm(tb32)}   {flop / median(tb32) / 1e9:.1f} TFLOP/s")
    print(f"  diinn_liif_backward_data_x3 (3 kernels)           {mmm(tbx3)}   {median(tb32) / median(tbx3):.2f}x; reads+writes {10 * plane_gb:.2f} GB"
          f" -> {10 * plane_gb / median(tbx3):.2f} TB/s")
    del acts, g, out, wk

    # gradient distances from float64 with pinned gates: each path's own planes, upcast, through the formula sheet
    db = min(dist_b, b)
    if db <= 0:                                                  # (--dist-batch=0: a large geometry, whose float64 planes would not fit)
        return
    f_s = feat.detach()[:db].clone().requires_grad_(True)
    r_s = r[:db].contiguous()
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    p64 = [p.detach().double() for p in ps]
    img, spl = LT.image_on_device(ps), LS.split_on_device(ps)
    cols = {}
    for tag, fn, planes in (("fp32", LT.LIIFFunction, lambda: LT.train_forward(f_s.detach().contiguous(), img, hu, wu)[1]),
                            ("split", LS.LIIFSplitFunction, lambda: LS.train_forward_split(f_s.detach().contiguous(), img, spl, hu, wu)[1])):
        saved = LT.saved_activations(planes(), db, hu, wu)
        hs = [saved[:, l].permute(0, 2, 1).double() for l in range(4)]
        del saved
        f_s.grad = None
        for p in ps:
            p.grad = None
        (fn.apply(f_s, hu, wu, *ps) * r_s).sum().backward()
        d64, g64 = LS.liif_backward_from_saved(r_s.double(), f_s.detach().double(), hs, p64, (hu, wu))
        del hs
        cols[tag] = [float((a.double() - ref).abs().max()) / float(ref.abs().max())
                     for a, ref in zip([f_s.grad] + [p.grad for p in ps], [d64] + g64)]
    print(f"  gradient distances at B={db} ({4 * db * hu * wu} virtual pixels)")
    print("  max|g - float64 on the path's own planes| / max|float64|:      fp32      split bf16")
    for i, name in enumerate(["feat"] + LT.PARAM_NAMES):
        print(f"    {name:18s}                              {cols['fp32'][i]:10.2e}    {cols['split'][i]:10.2e}")


if __name__ == "__main__":
    main()
