#!/usr/bin/env python3
"""Decoder ``init_q=True`` (mode 3) training step (decoder forward + backward) timing on one GPU.

  ours   : the decoder under autograd on the HIP path (initq_training.DecodeInitqFunction: initq_planes_kernel in radians +
           decode_kernel<SIN | DECODE_INITQ, true, SAVE> forward; bwd_layer_kernel, initq_bwd_kernel, the plane GEMMs / row products,
           cell_sum_rows_kernel and fold3x3_kernel backward)
  eager  : the reference's op sequence (diinn.py:113-115,132-139,163-173: first_layer + sin, F.unfold, nearest-exact replication,
           x' = E * X, the K / Q 1x1 convolutions on the materialised [B,576,Hu,Wu] tensor) in PyTorch-ROCm eager mode under
           autograd, restated inline (the reference itself is not a dependency of this repository)

The two alternate in one process, medians of ``--runs`` (20) single steps each.  Also printed: the forward under grad alone, the
backward's kernels one group at a time (events around the C ABI calls on the step's own buffers), initq_bwd_kernel's share of the
157.3 TFLOP/s fp32 matrix peak (2 x 640 x 1280 FLOP issued per pixel, 2 x 576 x 1280 useful), peak memory, the largest gradient
distance between the two paths and, at ``--dist-batch`` images (2), the HIP backward's distance from the float64 formula sheet given
the planes its own forward saved.  No time is asserted anywhere.

usage: initq_train_time.py [B] [LR] [SCALE] [--runs=N] [--dist-batch=N] [--only-ours] [--default-off]   (default 16 48 4: the reference's training patch)
       --only-ours:   5 steps of ours and nothing else, for a kernel trace
       --default-off: 5 mode-3 training steps (init_q=False) and 5 init_q inference forwards, the paths the switch leaves alone,
                      for a kernel trace to hold against the parent commit's
"""
import ctypes as C
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diinn_amd._native as N  # noqa: E402
import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.initq_training as IT  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402
import diinn_amd.training as T  # noqa: E402

PEAK = 157.3e12


def eager_forward(feat, p, size):
    """ImplicitDecoder.forward(x, size, None) with init_q=True, mode 3, in the reference's operators."""
    b, c, h, w = feat.shape
    hu, wu = size
    dev = feat.device
    idx_h, rel_h, idx_w, rel_w, ratio = T.coordinate_tensors(h, w, hu, wu, dev)
    syn = torch.empty((b, 3, hu, wu), device=dev)
    syn[:, 0] = rel_h[None, :, None]
    syn[:, 1] = rel_w[None, None, :]
    syn[:, 2] = ratio
    x = F.unfold(feat, 3, padding=1).view(b, c * 9, h, w)[:, :, idx_h][:, :, :, idx_w]
    e = torch.sin(F.conv2d(syn, p["first_layer.0.weight"], p["first_layer.0.bias"]))
    x = x * e
    k = torch.relu(F.conv2d(x, p["K.0.0.weight"], p["K.0.0.bias"]))
    q = k * torch.sin(F.conv2d(e, p["Q.0.0.weight"], p["Q.0.0.bias"]))
    for i in (1, 2, 3):
        k = torch.relu(F.conv2d(torch.cat([q, x], 1), p[f"K.{i}.0.weight"], p[f"K.{i}.0.bias"]))
        q = k * torch.sin(F.conv2d(q, p[f"Q.{i}.0.weight"], p[f"Q.{i}.0.bias"]))
    return F.conv2d(q, p["last_layer.weight"], p["last_layer.bias"])


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


def default_off(b, lr, hu, wu, dev):
    sd3 = synth.decoder_state_dict(123, 1.0, mode=3)
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)
    dec3 = D.ImplicitDecoder(mode=3)
    dec3.load_state_dict({k: torch.from_numpy(v) for k, v in sd3.items()}, strict=True)
    dec3 = dec3.to(dev).train()
    for _ in range(5):
        dec3.zero_grad(set_to_none=True)
        feat.grad = None
        (dec3(feat, (hu, wu)) * r).sum().backward()
    sdq = synth.decoder_state_dict(123, 1.0, mode=3, init_q=True)
    decq = D.ImplicitDecoder(mode=3, init_q=True)
    decq.load_state_dict({k: torch.from_numpy(v) for k, v in sdq.items()}, strict=True)
    decq = decq.to(dev).eval()
    with torch.no_grad():
        for _ in range(5):
            decq(feat.detach(), (hu, wu))
    torch.cuda.synchronize()


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
    print(f"init_q decoder (mode 3)  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels, {b * lr * lr} cells; device {torch.cuda.get_device_name(0)}")
    if "--default-off" in sys.argv:
        default_off(b, lr, hu, wu, dev)
        return
    sd = synth.decoder_state_dict(123, 1.0, mode=3, init_q=True)
    named = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sd.items()}
    params = [named[k] for k in IT.INITQ_PARAM_NAMES]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)

    def zero():
        feat.grad = None
        for p in params:
            p.grad = None

    def ours_step():
        zero()
        (IT.DecodeInitqFunction.apply(feat, hu, wu, N.SIN_DEFAULT, *params) * r).sum().backward()

    if "--only-ours" in sys.argv:
        for _ in range(5):
            ours_step()
        torch.cuda.synchronize()
        return

    def eager_step():
        zero()
        (eager_forward(feat, named, (hu, wu)) * r).sum().backward()

    def ours_fwd_grad():
        IT.DecodeInitqFunction.apply(feat, hu, wu, N.SIN_DEFAULT, *params)

    for fn in (ours_step, eager_step, ours_fwd_grad):
        fn()
        fn()
    ours_step()
    g_ours = [feat.grad.clone()] + [p.grad.clone() for p in params]
    eager_step()
    g_eager = [feat.grad.clone()] + [p.grad.clone() for p in params]
    cross = [(float((a - e).abs().max()) / float(e.abs().max()), name) for name, a, e in zip(["feat"] + IT.INITQ_PARAM_NAMES, g_ours, g_eager)]
    del g_ours, g_eager
    torch.cuda.reset_peak_memory_stats()
    ours_step()
    torch.cuda.synchronize()
    peak_ours = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    eager_step()
    torch.cuda.synchronize()
    peak_eager = torch.cuda.max_memory_allocated()
    t_ours, t_eager, t_f1 = [], [], []
    for _ in range(runs):
        t_ours.append(once(ours_step))
        t_eager.append(once(eager_step))
        t_f1.append(once(ours_fwd_grad))
    print(f"  forward under grad (planes + decode_kernel<SAVE>)  {median(t_f1):8.2f} ms")
    print(f"  step fwd+bwd, HIP path                             {median(t_ours):8.2f} ms   (min {min(t_ours):.2f}, max {max(t_ours):.2f}; {runs} runs)")
    print(f"  step fwd+bwd, reference op sequence (eager)        {median(t_eager):8.2f} ms   (min {min(t_eager):.2f}, max {max(t_eager):.2f})   "
          f"eager / HIP = {median(t_eager) / median(t_ours):.2f}")
    print(f"  backward = step - forward under grad               {median(t_ours) - median(t_f1):8.2f} ms")
    print(f"  peak memory: HIP path {peak_ours / 2**30:.2f} GiB, eager {peak_eager / 2**30:.2f} GiB")
    print(f"  largest max|g_hip - g_eager| / max|g_eager| over the 21 gradients: {max(cross)[0]:.2e} ({max(cross)[1]}); this figure includes "
          f"the ReLU gates that fall differently in the two fp32 forwards (at this size some pre-activation always lies within fp32 noise of zero)")
    # the HIP backward against the float64 formula sheet GIVEN the planes its own forward saved, at a smaller batch: no gate luck
    db = min(dist_b, b)
    ps = [p.detach() for p in params]
    f_s, r_s = feat.detach()[:db].contiguous(), r[:db].contiguous()
    _, acts_s, packed_s, image_s = IT.train_forward_initq(f_s, ps, hu, wu, N.SIN_DEFAULT)
    d_f, d_p = IT.backward_fused_initq(r_s, f_s, acts_s, packed_s, image_s, (hu, wu))
    plain = T.untile_planes(acts_s, db * hu * wu).reshape(4, 2, 256, -1).double()
    w_f, w_p = IT.backward_from_saved_initq(r_s.double(), f_s.double(), plain, [p.double() for p in ps], (hu, wu))
    dist = [(float((a.double() - e).abs().max()) / float(e.abs().max()), name) for name, a, e in zip(["feat"] + IT.INITQ_PARAM_NAMES, [d_f] + d_p, [w_f] + w_p)]
    print(f"  largest max|g_hip - float64 given the saved planes| / max|float64| at B={db} ({db * hu * wu} pixels): {max(dist)[0]:.2e} ({max(dist)[1]})")
    del acts_s, plain, d_f, d_p, w_f, w_p

    # the backward's kernels, one group at a time, on buffers of the step's shapes
    lib = N.load()
    feat_c = feat.detach().contiguous()
    out, acts, packed, image = IT.train_forward_initq(feat_c, [p.detach() for p in params], hu, wu, N.SIN_DEFAULT)
    t = (n + 31) // 32
    gp = r.permute(1, 0, 2, 3).reshape(3, n).contiguous()
    g = torch.empty((4, t, 512, 32), device=dev)
    q = torch.empty((4, t, 256, 32), device=dev)
    u_t, da_t = torch.empty((t, 576, 32), device=dev), torch.empty((t, 576, 32), device=dev)
    xp_t, e_t = torch.empty((t, 640, 32), device=dev), torch.empty((t, 640, 32), device=dev)
    geo = T._geometry(b, lr, lr, hu, wu, dev)
    ks, xs = max(1, min(T.WGRAD_KSPLIT, t)), max(1, min(IT.WGRAD_X_KSPLIT, t))
    part = torch.empty((3, ks, 512, 257), device=dev)
    partx = torch.empty((5, xs, 640, 256), device=dev)
    d_unf = torch.empty((b, 576, lr, lr), device=dev)
    d_feat = torch.empty((b, 64, lr, lr), device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def k_fwd():
        IT.train_forward_initq(feat_c, [p.detach() for p in params], hu, wu, N.SIN_DEFAULT)

    def k_data():
        N.check(lib.diinn_backward_data(stream, ptr(gp), ptr(acts), ptr(packed), ptr(g), ptr(q), n), "diinn_backward_data")

    def k_gemm():
        for i in (3, 2, 1):
            N.check(lib.diinn_plane_gemm_nt(stream, ptr(g[i]), 512, 0, ptr(q[i - 1]), 256, 0, ptr(part[i - 1]), 512, 256, n, ks, 1), "diinn_plane_gemm_nt")

    def k_initq():
        N.check(lib.diinn_initq_backward(stream, ptr(feat_c), ptr(g), ptr(image), ptr(u_t), ptr(da_t), ptr(xp_t), ptr(e_t), b, lr, lr, hu, wu),
                "diinn_initq_backward")

    def k_xgemm():
        for i in range(4):
            N.check(lib.diinn_plane_gemm_nt(stream, ptr(xp_t), 640, 0, ptr(g[i]), 512, 0, ptr(partx[i]), 640, 256, n, xs, 0), "diinn_plane_gemm_nt")
        N.check(lib.diinn_plane_gemm_nt(stream, ptr(e_t), 640, 0, ptr(g[0]), 512, 256, ptr(partx[4]), 640, 256, n, xs, 0), "diinn_plane_gemm_nt")

    def k_cells():
        N.check(lib.diinn_cell_sum_rows(stream, ptr(u_t), 576, 576, ptr(geo["seg_h"]), ptr(geo["seg_w"]), ptr(d_unf), b, lr, lr, hu, wu), "diinn_cell_sum_rows")
        N.check(lib.diinn_fold3x3(stream, ptr(d_unf), ptr(d_feat), b, 64, lr, lr), "diinn_fold3x3")

    t_fwd, t_data, t_gemm = timed(k_fwd, runs), timed(k_data, runs), timed(k_gemm, runs)
    t_initq, t_xgemm, t_cell = timed(k_initq, runs), timed(k_xgemm, runs), timed(k_cells, runs)
    f_chain, f_init, f_init_useful = 3 * 2.0 * 512 * 256 * n, 2.0 * 640 * 1280 * n, 2.0 * 576 * 1280 * n
    print(f"  diinn_decode_initq_train_fwd (2 kernels, + gathers) {t_fwd:8.3f} ms")
    print(f"  diinn_backward_data (3 kernels)                     {t_data:8.3f} ms   {f_chain / t_data / 1e9:.1f} TFLOP/s")
    print(f"  3 x diinn_plane_gemm_nt [dWq ; dQw | db]            {t_gemm:8.3f} ms   {f_chain / t_gemm / 1e9:.1f} TFLOP/s")
    print(f"  diinn_initq_backward (initq_bwd_kernel)             {t_initq:8.3f} ms   issued {f_init / t_initq / 1e9:.1f} TFLOP/s = {f_init / t_initq * 1e3 / PEAK:.3f} of peak; "
          f"useful {f_init_useful / t_initq / 1e9:.1f} TFLOP/s = {f_init_useful / t_initq * 1e3 / PEAK:.3f}")
    print(f"  5 x diinn_plane_gemm_nt [dWx_i^T, dQ0^T] (640 rows) {t_xgemm:8.3f} ms   {f_init / t_xgemm / 1e9:.1f} TFLOP/s = {f_init / t_xgemm * 1e3 / PEAK:.3f} of peak")
    print(f"  diinn_cell_sum_rows + diinn_fold3x3                 {t_cell:8.3f} ms   reads {t * 576 * 128 / 1e9:.2f} GB -> {t * 576 * 128 / 1e9 / t_cell:.2f} TB/s")
    print(f"  rest of the backward (row products, partial sums, glue) {median(t_ours) - median(t_f1) - t_data - t_gemm - t_initq - t_xgemm - t_cell:8.3f} ms")


if __name__ == "__main__":
    main()
