#!/usr/bin/env python3
"""MetaSR decoder training step (forward + backward) timing on one GPU.

  ours   : the decoder under autograd on the HIP path (metasr_training.MetaSRFunction: the inference kernels + M on the hoisted-conv
           kernel forward; metasr_bwd_cells_kernel + the library's conv-gradient kernels backward)
  eager  : the reference's op sequence (metasr.py:70-104: unfold -> nearest gather -> Linear, ReLU, Linear -> view -> bmm) in
           PyTorch-ROCm eager mode under autograd, restated inline (the reference itself does not travel to the GPU box)

The two alternate in one process, medians of ``--runs`` (20) single steps each.  Also printed: the forward alone (no_grad and
under grad), diinn_metasr_backward_cells alone with its achieved bytes/s against its algorithmic bytes, and every gradient's
distance from float64 (the formula sheet in float64 on the GPU) for both paths.

usage: metasr_train_time.py [B] [LR] [SCALE] [--runs=N] [--only-ours]     (default 16 48 4: the reference's training patch geometry)
       --only-ours: 7 steps of ours and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/metasr_train_time.py --only-ours)
"""
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diinn_amd.metasr_training as MT  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

SHAPES = {"imnet.layers.0.weight": (256, 3), "imnet.layers.0.bias": (256,),
          "imnet.layers.2.weight": (1728, 256), "imnet.layers.2.bias": (1728,)}


def eager_forward(feat, params, cell, inp, size):
    """query_rgb + reshape_pred: the per-pixel gather of the unfolded features stands for grid_sample(mode='nearest')."""
    w1, b1, w2, b2 = params
    b, c, h, w = feat.shape
    u = F.unfold(feat, 3, padding=1).permute(0, 2, 1).reshape(b * h * w, c * 9)
    q_feat = u[cell]                                              # [N, 576]
    pred = F.linear(torch.relu(F.linear(inp, w1, b1)), w2, b2).view(-1, c * 9, 3)
    pred = torch.bmm(q_feat.view(-1, 1, c * 9), pred)
    return pred.view(b, size[0], size[1], 3).permute(0, 3, 1, 2).contiguous()


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    argv = [a for a in sys.argv if not a.startswith("--")]
    runs = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--runs=")), 20)
    only_ours = "--only-ours" in sys.argv
    b = int(argv[1]) if len(argv) > 1 else 16
    lr = int(argv[2]) if len(argv) > 2 else 48
    sc = int(argv[3]) if len(argv) > 3 else 4
    hu = wu = lr * sc
    dev = torch.device("cuda:0")
    sd = synth.state_dict_for(SHAPES, 123, "metasr.")
    params = [torch.from_numpy(sd["imnet." + n]).to(dev).requires_grad_(True) for n in MT.PARAM_NAMES]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)
    n, cells = b * hu * wu, b * lr * lr

    def zero():
        feat.grad = None
        for p in params:
            p.grad = None

    def ours_step():
        zero()
        (MT.MetaSRFunction.apply(feat, hu, wu, *params) * r).sum().backward()

    print(f"MetaSR decoder  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels, {cells} cells")
    if only_ours:
        for _ in range(7):
            ours_step()
        torch.cuda.synchronize()
        return

    cell, inp = MT._pixel_tables(b, lr, lr, hu, wu, dev, torch.float32)

    def eager_step():
        zero()
        (eager_forward(feat, params, cell, inp, (hu, wu)) * r).sum().backward()

    def ours_fwd_nograd():
        with torch.no_grad():
            from diinn_amd.decoder import metasr_decode_features
            metasr_decode_features(feat.detach(), MT.images_on_device(params)[0], (hu, wu))

    def ours_fwd_grad():
        MT.MetaSRFunction.apply(feat, hu, wu, *params)

    for fn in (ours_step, eager_step, ours_fwd_nograd, ours_fwd_grad):
        fn()
        fn()
    t_ours, t_eager, t_f0, t_f1 = [], [], [], []
    for _ in range(runs):
        t_ours.append(once(ours_step))
        t_eager.append(once(eager_step))
        t_f0.append(once(ours_fwd_nograd))
        t_f1.append(once(ours_fwd_grad))
    print(f"  forward, no_grad (unfold + metasr_kernel)       {median(t_f0):8.2f} ms")
    print(f"  forward under grad (+ M on the hoisted conv)     {median(t_f1):8.2f} ms")
    print(f"  step fwd+bwd, HIP path                           {median(t_ours):8.2f} ms   (min {min(t_ours):.2f}, max {max(t_ours):.2f}; {runs} runs)")
    print(f"  step fwd+bwd, reference op sequence (eager)      {median(t_eager):8.2f} ms   (min {min(t_eager):.2f}, max {max(t_eager):.2f})   {median(t_eager) / median(t_ours):.2f}x")
    print(f"  backward = step - forward under grad             {median(t_ours) - median(t_f1):8.2f} ms   = {100 * (median(t_ours) - median(t_f1)) / median(t_f1):.0f} % of the forward")

    # the new kernel alone (with the add of its layer-0 partials)
    packed, image, wx = MT.images_on_device(params)
    m = torch.randn(b, lr, lr, 1024, device=dev)
    for _ in range(3):
        MT.backward_cells(r, m, packed, (hu, wu))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for e0, e1 in ev:
        e0.record()
        MT.backward_cells(r, m, packed, (hu, wu))
        e1.record()
    torch.cuda.synchronize()
    t_k = median([e0.elapsed_time(e1) for e0, e1 in ev])
    tiles = (cells + 31) // 32
    nbytes = cells * 3 * 256 * 4 + 2 * tiles * 32 * 1024 * 4 + n * 12 + 2 * tiles * 4096
    print(f"  diinn_metasr_backward_cells + diinn_sum_parts    {t_k:8.3f} ms   algorithmic bytes {nbytes / 1e6:.1f} MB -> {nbytes / t_k / 1e9:.2f} TB/s")

    # gradient distances from float64
    ours_step()
    g_ours = [feat.grad.clone()] + [p.grad.clone() for p in params]
    eager_step()
    g_eager = [feat.grad.clone()] + [p.grad.clone() for p in params]
    d_feat, g64 = MT.metasr_backward_reference(r.double(), feat.detach().double(), [p.detach().double() for p in params], (hu, wu))
    print("  max|g - float64| / max|float64|:      HIP path      eager fp32")
    for name, a, e, t in zip(["feat"] + MT.PARAM_NAMES, g_ours, g_eager, [d_feat] + g64):
        s = float(t.abs().max())
        print(f"    {name:18s}              {float((a.double() - t).abs().max()) / s:10.2e}    {float((e.double() - t).abs().max()) / s:10.2e}")
    print(f"  peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


if __name__ == "__main__":
    main()
