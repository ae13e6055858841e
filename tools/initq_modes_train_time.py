#!/usr/bin/env python3
"""Decoder ``init_q=True`` with modes 1, 2 and 4: training step (decoder forward + backward) timing on one GPU.

  ours   : the decoder under autograd on the HIP path (initq_modes_training.DecodeInitqModesFunction)
  eager  : the reference's op sequence (diinn.py:113-147,163-173: first_layer + sin, F.unfold, nearest-exact replication,
           x' = E * X, the K / Q 1x1 convolutions on the materialised [B,576,Hu,Wu] tensor, mode 4's reflect-padded 3x3 head) in
           PyTorch-ROCm eager mode under autograd, restated inline (the reference itself is not a dependency of this repository)

Per mode the two alternate in one process, medians of ``--runs`` (20) single steps each; mode 3 with ``init_q`` (the step this path
must leave alone) is timed in the same process for the comparison.  Also printed: peak memory of both, the largest gradient
distance between the two paths, and pixel_chain_bwd_kernel alone beside cell_chain_bwd_kernel on the same count of records, with
their shares of the 157.3 TFLOP/s fp32 matrix peak (3 x 2 x 256 x 256 FLOP per record).  No time is asserted anywhere.

usage: initq_modes_train_time.py [B] [LR] [SCALE] [--runs=N]      (default 16 48 4: the reference's training patch)
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
import diinn_amd.initq_modes_training as MT  # noqa: E402
import diinn_amd.initq_training as IT  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402
import diinn_amd.training as T  # noqa: E402

PEAK = 157.3e12


def eager_forward(feat, p, size, mode):
    """ImplicitDecoder.forward(x, size, None) with init_q=True in the reference's operators."""
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
        kin = k if mode == 1 else torch.cat([k if mode == 2 else q, x], 1)
        k = torch.relu(F.conv2d(kin, p[f"K.{i}.0.weight"], p[f"K.{i}.0.bias"]))
        q = k * torch.sin(F.conv2d(q, p[f"Q.{i}.0.weight"], p[f"Q.{i}.0.bias"]))
    if mode == 4:
        return F.conv2d(F.pad(q, (1, 1, 1, 1), mode="reflect"), p["last_layer.weight"], p["last_layer.bias"])
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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2**30


def step_times(mode, b, lr, hu, wu, runs, dev):
    sd = synth.decoder_state_dict(123, 1.0, mode=mode, init_q=True)
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
        if mode == 3:
            out = IT.DecodeInitqFunction.apply(feat, hu, wu, N.SIN_DEFAULT, *params)
        else:
            out = MT.DecodeInitqModesFunction.apply(feat, hu, wu, N.SIN_DEFAULT, mode, *params)
        (out * r).sum().backward()

    def eager_step():
        zero()
        (eager_forward(feat, named, (hu, wu), mode) * r).sum().backward()

    for fn in (ours_step, eager_step):
        fn()
        fn()
    ours_step()
    g_ours = [feat.grad.clone()] + [p.grad.clone() for p in params]
    eager_step()
    g_eager = [feat.grad.clone()] + [p.grad.clone() for p in params]
    cross = max((float((a - e).abs().max()) / float(e.abs().max()), name)
                for name, a, e in zip(["feat"] + IT.INITQ_PARAM_NAMES, g_ours, g_eager))
    del g_ours, g_eager
    peak_ours, peak_eager = peak_of(ours_step), peak_of(eager_step)
    t_ours, t_eager = [], []
    for _ in range(runs):
        t_ours.append(once(ours_step))
        t_eager.append(once(eager_step))
    print(f"  mode {mode} + init_q   step fwd+bwd: HIP path {median(t_ours):8.2f} ms (min {min(t_ours):.2f}, max {max(t_ours):.2f}; {runs} runs)   "
          f"eager {median(t_eager):8.2f} ms (min {min(t_eager):.2f}, max {max(t_eager):.2f})   eager / HIP = {median(t_eager) / median(t_ours):.2f}")
    print(f"                      peak memory: HIP path {peak_ours:.2f} GiB, eager {peak_eager:.2f} GiB;   largest max|g_hip - g_eager| / max|g_eager| "
          f"{cross[0]:.2e} ({cross[1]}; includes the ReLU gates that fall differently in the two fp32 forwards)")
    zero()
    return median(t_ours), median(t_eager)


def chain_kernels(records, runs, dev):
    """pixel_chain_bwd_kernel on ``records`` HR pixels beside cell_chain_bwd_kernel on as many LR cells (B = 1, H = 1, W = records)."""
    lib = N.load()
    sd = synth.decoder_state_dict(123, 1.0, mode=3, init_q=True)
    packed = IT.pack_body_on_device({k: torch.from_numpy(v).to(dev) for k, v in sd.items()})
    t = (records + 31) // 32
    g = torch.randn((4, t, 512, 32), device=dev)
    acts = torch.randn((4, t, 512, 32), device=dev)
    s_t = torch.randn((t, 1024, 32), device=dev)
    chain = torch.randn((records, 1024), device=dev)
    dp = torch.empty((1, 1024, 1, records), device=dev)
    k_t = torch.empty((t, 768, 32), device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t_pix = timed(lambda: N.check(lib.diinn_pixel_chain_bwd(stream, ptr(g), ptr(acts), ptr(packed), records), "diinn_pixel_chain_bwd"), runs)
    t_cell = timed(lambda: N.check(lib.diinn_cell_chain_bwd(stream, ptr(s_t), ptr(chain), ptr(packed), ptr(dp), ptr(s_t), ptr(k_t), 1, 1, records),
                                   "diinn_cell_chain_bwd"), runs)
    flop = 3 * 2.0 * 256 * 256 * records
    print(f"  pixel_chain_bwd_kernel on {records} pixels {t_pix:8.3f} ms   {flop / t_pix / 1e9:.1f} TFLOP/s = {flop / t_pix * 1e3 / PEAK:.3f} of the fp32 matrix peak "
          f"(reads 3 x 2 and writes 3 x 1 KiB-rows of planes per pixel: {records * 9 * 1024 / 1e9:.2f} GB -> {records * 9 * 1024 / 1e9 / t_pix:.2f} TB/s)")
    print(f"  cell_chain_bwd_kernel  on {records} cells  {t_cell:8.3f} ms   {flop / t_cell / 1e9:.1f} TFLOP/s = {flop / t_cell * 1e3 / PEAK:.3f} of the fp32 matrix peak "
          f"(both layouts of dP and k_0..k_2 written)")


def main():
    argv = [a for a in sys.argv if not a.startswith("--")]
    runs = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--runs=")), 20)
    b = int(argv[1]) if len(argv) > 1 else 16
    lr = int(argv[2]) if len(argv) > 2 else 48
    sc = int(argv[3]) if len(argv) > 3 else 4
    hu = wu = lr * sc
    dev = torch.device("cuda:0")
    n = b * hu * wu
    print(f"init_q decoder, modes 1, 2, 4 (and 3)  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels, {b * lr * lr} cells; device {torch.cuda.get_device_name(0)}")
    for mode in (3, 1, 2, 4):
        step_times(mode, b, lr, hu, wu, runs, dev)
        torch.cuda.empty_cache()
    chain_kernels(n, runs, dev)


if __name__ == "__main__":
    main()
