#!/usr/bin/env python3
"""Decoder mode 4 training step (decoder forward + backward) timing on one GPU, against mode 3 on the same build.

  mode 4 : the decoder under autograd on the HIP path (mode4_training.DecodeMode4Function: mode 3's training forward on the body
           image, head3x3_taps_from_planes_kernel + head3x3_reflect_kernel; bwd_head3x3_kernel + 3 x bwd_layer_kernel, seven row
           products for the head's weight gradient, the rest mode 3's backward)
  mode 3 : training.DecodeMode3Function with the same K / Q weights and a 1x1 head (the fused-head form of the backward)
  eager  : the reference's op sequence for mode 4 (diinn.py:132-147,163-173: F.unfold, nearest-exact replication, the K / Q 1x1
           convolutions on the materialised [B,576,Hu,Wu] tensor, the reflect-padded 3x3 head) in PyTorch-ROCm eager mode under
           autograd, restated inline (mode4_training.forward_torch_mode4; the reference itself is not a dependency of this repository)

The three alternate in one process, medians of ``--runs`` (20) single steps each.  Also printed: the forwards under grad alone, the
kernels mode 4 adds one group at a time (events around the C ABI calls on the step's own buffers) with the bytes they move -- the
forward's head reads 2 KiB per pixel (k_3, s_3) and writes 112 B of taps; the backward's reads 2 KiB and writes 3 KiB (G_3, q_3)
plus 112 B of dT -- next to mode 3's diinn_backward_data, whose fused head never reads G_3 back; peak memory; the largest gradient
distance between mode 4 and the eager path.  No time is asserted anywhere.

usage: mode4_train_time.py [B] [LR] [SCALE] [--runs=N] [--only-ours]   (default 16 48 4: the reference's training patch)
       --only-ours: 5 mode-4 steps and nothing else, for a kernel trace
"""
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diinn_amd._native as N  # noqa: E402
import diinn_amd.mode4_training as M4  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402
import diinn_amd.training as T  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    return sorted(xs)[len(xs) // 2]


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


def main():
    argv = [a for a in sys.argv if not a.startswith("--")]
    runs = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--runs=")), 20)
    b = int(argv[1]) if len(argv) > 1 else 16
    lr = int(argv[2]) if len(argv) > 2 else 48
    sc = int(argv[3]) if len(argv) > 3 else 4
    hu = wu = lr * sc
    dev = torch.device("cuda:0")
    n = b * hu * wu
    print(f"decoder mode 4 against mode 3  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels, {b * lr * lr} cells; device {torch.cuda.get_device_name(0)}")
    sd4 = synth.decoder_state_dict(123, 1.0, mode=4)
    sd3 = synth.decoder_state_dict(123, 1.0, mode=3)
    named4 = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sd4.items()}
    p4 = [named4[k] for k in T.PARAM_NAMES]
    # mode 3 on the same K / Q weights; its own 1x1 head
    p3 = [*p4[:16], *[torch.from_numpy(sd3[k]).to(dev).requires_grad_(True) for k in T.PARAM_NAMES[16:]]]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)

    def zero():
        feat.grad = None
        for p in (*p4, *p3[16:]):
            p.grad = None

    def m4_step():
        zero()
        (M4.DecodeMode4Function.apply(feat, hu, wu, N.SIN_DEFAULT, *p4) * r).sum().backward()

    if "--only-ours" in sys.argv:
        for _ in range(5):
            m4_step()
        torch.cuda.synchronize()
        return

    def m3_step():
        zero()
        (T.DecodeMode3Function.apply(feat, hu, wu, N.SIN_DEFAULT, *p3) * r).sum().backward()

    def eager_step():
        zero()
        (M4.forward_torch_mode4(feat, p4, (hu, wu))[0] * r).sum().backward()

    def m4_fwd():
        M4.DecodeMode4Function.apply(feat, hu, wu, N.SIN_DEFAULT, *p4)

    def m3_fwd():
        T.DecodeMode3Function.apply(feat, hu, wu, N.SIN_DEFAULT, *p3)

    for fn in (m4_step, m3_step, eager_step, m4_fwd, m3_fwd):
        fn()
        fn()
    m4_step()
    g_ours = [feat.grad.clone()] + [p.grad.clone() for p in p4]
    eager_step()
    g_eager = [feat.grad.clone()] + [p.grad.clone() for p in p4]
    cross = [(float((a - e).abs().max()) / float(e.abs().max()), name) for name, a, e in zip(["feat"] + T.PARAM_NAMES, g_ours, g_eager)]
    del g_ours, g_eager
    peaks = []
    for fn in (m4_step, m3_step, eager_step):
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
    t4, t3, te, f4, f3 = [], [], [], [], []
    for _ in range(runs):
        t4.append(once(m4_step))
        t3.append(once(m3_step))
        te.append(once(eager_step))
        f4.append(once(m4_fwd))
        f3.append(once(m3_fwd))
    print(f"  forward under grad, mode 4 / mode 3                {median(f4):8.2f} / {median(f3):.2f} ms   (difference {median(f4) - median(f3):+.2f})")
    print(f"  step fwd+bwd, mode 4 on the HIP path               {median(t4):8.2f} ms   (min {min(t4):.2f}, max {max(t4):.2f}; {runs} runs)")
    print(f"  step fwd+bwd, mode 3 on the HIP path               {median(t3):8.2f} ms   (min {min(t3):.2f}, max {max(t3):.2f})   "
          f"mode 4 - mode 3 = {median(t4) - median(t3):+.2f} ms = {100 * (median(t4) / median(t3) - 1):+.1f} %")
    print(f"  step fwd+bwd, reference op sequence (eager)        {median(te):8.2f} ms   (min {min(te):.2f}, max {max(te):.2f})   "
          f"eager / HIP = {median(te) / median(t4):.2f}")
    print(f"  peak memory: mode 4 {peaks[0] / 2**30:.2f} GiB, mode 3 {peaks[1] / 2**30:.2f} GiB, eager {peaks[2] / 2**30:.2f} GiB")
    print(f"  largest max|g_hip - g_eager| / max|g_eager| over the 19 gradients: {max(cross)[0]:.2e} ({max(cross)[1]}); this figure includes "
          f"the ReLU gates that fall differently in the two fp32 forwards")

    # what mode 4 adds, one group at a time, on buffers of the step's shapes
    lib = N.load()
    feat_c = feat.detach().contiguous()
    d4 = [p.detach() for p in p4]
    out, acts, body, head = M4.train_forward_mode4(feat_c, d4, hu, wu, N.SIN_DEFAULT)
    packed3 = T.pack_on_device([p.detach() for p in p3])
    t = (n + 31) // 32
    gp = r.permute(1, 0, 2, 3).reshape(3, n).contiguous()
    g = torch.empty((4, t, 512, 32), device=dev)
    q = torch.empty((4, t, 256, 32), device=dev)
    dt = torch.zeros((7, t, 4, 32), device=dev)
    taps = torch.empty(n * 28, device=dev)
    rs = max(1, min(T.ROWDOT_SPLITS, t))
    partl = torch.empty((7, rs, 256, 4), device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def k_head_fwd():
        N.check(lib.diinn_head3x3_from_planes(stream, ptr(acts), ptr(body), ptr(head), ptr(taps), ptr(out), b, hu, wu), "diinn_head3x3_from_planes")

    def k_data4():
        N.check(lib.diinn_backward_data_head3x3(stream, ptr(gp), ptr(acts), ptr(body), ptr(head), ptr(g), ptr(q), ptr(dt), b, hu, wu),
                "diinn_backward_data_head3x3")

    def k_data3():
        N.check(lib.diinn_backward_data(stream, ptr(gp), ptr(acts), ptr(packed3), ptr(g), ptr(q), n), "diinn_backward_data")

    def k_rowdot(count):
        def run():
            for i in range(count):
                N.check(lib.diinn_plane_rowdot(stream, ptr(q[3]), 256, ptr(dt[i]), ptr(partl[i]), 256, n, rs), "diinn_plane_rowdot")
        return run

    t_hf, t_d4, t_d3 = timed(k_head_fwd, runs), timed(k_data4, runs), timed(k_data3, runs)
    t_r7, t_r1 = timed(k_rowdot(7), runs), timed(k_rowdot(1), runs)
    fwd_b, bwd_b = n * (2048 + 112 + 9 * 12 + 12), n * (2048 + 3072 + 112 + 12)
    print(f"  diinn_head3x3_from_planes (taps from planes + gather) {t_hf:8.3f} ms   moves {fwd_b / 1e9:.2f} GB -> {fwd_b / 1e9 / t_hf:.2f} TB/s")
    print(f"  diinn_backward_data_head3x3 (4 kernels)               {t_d4:8.3f} ms")
    print(f"  diinn_backward_data, mode 3 (3 kernels, fused head)   {t_d3:8.3f} ms   difference {t_d4 - t_d3:+.3f} ms; bwd_head3x3_kernel moves "
          f"{bwd_b / 1e9:.2f} GB and layer 3's kernel reads G_3 back ({n * 2048 / 1e9:.2f} GB) where the fused head reads k_3, s_3 once")
    print(f"  7 x diinn_plane_rowdot (dLw) / 1 x (mode 3's dL)      {t_r7:8.3f} / {t_r1:.3f} ms   each reads q_3, {n * 1024 / 1e9:.2f} GB")


if __name__ == "__main__":
    main()
