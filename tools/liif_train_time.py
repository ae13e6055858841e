#!/usr/bin/env python3
"""LIIF decoder training step (forward + backward) timing on one GPU.

  ours   : the decoder under autograd on the HIP path (liif_training.LIIFFunction: the inference kernels saving h_1..h_4 forward;
           liif_bwd_layer_kernel, the plane GEMMs / row products, liif_cell_sum_kernel and the library's conv-gradient kernels backward)
  eager  : the reference's op sequence (liif.py:59-127: unfold -> four nearest grid_sample gathers -> the 5-layer MLP -> area blend)
           in PyTorch-ROCm eager mode under autograd, restated inline (the reference itself does not travel to the GPU box)

The two alternate in one process, medians of ``--runs`` (10) single steps each.  Also printed: the forward alone (no_grad and
under grad), the backward's kernels one group at a time (events around the C ABI calls on the step's own buffers), and every
gradient's distance from float64 for both paths at ``--dist-batch`` images (2): the formula sheet in float64 on the GPU GIVEN the
path's own ReLU masks (at these sizes some pre-activation always lies within fp32 noise of zero; a direct comparison would
measure mask luck).  No time is asserted anywhere.

usage: liif_train_time.py [B] [LR] [SCALE] [--runs=N] [--dist-batch=N] [--only-ours]   (default 16 48 4: the reference's training patch geometry)
       --only-ours: 5 steps of ours and nothing else, for a kernel trace
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
import diinn_amd.liif_training as LT  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402
import diinn_amd.training as T  # noqa: E402

SHAPES = {"imnet.layers.0.weight": (256, 580), "imnet.layers.0.bias": (256,),
          **{f"imnet.layers.{i}.weight": (256, 256) for i in (2, 4, 6)}, **{f"imnet.layers.{i}.bias": (256,) for i in (2, 4, 6)},
          "imnet.layers.8.weight": (3, 256), "imnet.layers.8.bias": (3,)}


def centres(n, dev):
    return -1 + (2 * torch.arange(n, device=dev).float() + 1) / n


def eager_forward(feat, params, size, keep=None):
    """query_rgb + reshape_pred with the reference's operators: F.unfold, grid_sample(mode='nearest') of the unfolded features and
    of the cell-centre map per ensemble shift, the Linear / ReLU stack, the blend by the opposite areas.  ``keep``: a list that
    receives the hidden activations [member][layer] (for the masks)."""
    b, c, h, w = feat.shape
    hu, wu = size
    dev = feat.device
    u = F.unfold(feat, 3, padding=1).view(b, c * 9, h, w)
    coord = torch.stack(torch.meshgrid(centres(hu, dev), centres(wu, dev), indexing="ij"), dim=-1).view(1, -1, 2).expand(b, -1, -1)
    fcoord = torch.stack(torch.meshgrid(centres(h, dev), centres(w, dev), indexing="ij"), dim=-1).permute(2, 0, 1).unsqueeze(0).expand(b, 2, h, w)
    cell = torch.tensor([2.0 / hu * h, 2.0 / wu * w], device=dev).view(1, 1, 2).expand(b, coord.shape[1], 2)
    preds, areas = [], []
    for vx in (-1, 1):
        for vy in (-1, 1):
            c_ = coord.clone()
            c_[:, :, 0] += vx / h + 1e-6
            c_[:, :, 1] += vy / w + 1e-6
            c_.clamp_(-1 + 1e-6, 1 - 1e-6)
            grid = c_.flip(-1).unsqueeze(1)
            q_feat = F.grid_sample(u, grid, mode="nearest", align_corners=False)[:, :, 0, :].permute(0, 2, 1)
            q_coord = F.grid_sample(fcoord, grid, mode="nearest", align_corners=False)[:, :, 0, :].permute(0, 2, 1)
            rel = coord - q_coord
            rel = rel * torch.tensor([float(h), float(w)], device=dev)
            x = torch.cat([q_feat, rel, cell], dim=-1).view(b * coord.shape[1], -1)
            hid = []
            for l in range(4):
                x = torch.relu(F.linear(x, params[2 * l], params[2 * l + 1]))
                hid.append(x)
            if keep is not None:
                keep.append(hid)
            preds.append(F.linear(x, params[8], params[9]).view(b, -1, 3))
            areas.append((rel[:, :, 0] * rel[:, :, 1]).abs() + 1e-9)
    tot = torch.stack(areas).sum(dim=0)
    areas = areas[::-1]
    ret = 0
    for pred, area in zip(preds, areas):
        ret = ret + pred * (area / tot).unsqueeze(-1)
    return ret.view(b, hu, wu, 3).permute(0, 3, 1, 2).contiguous()


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
    runs = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--runs=")), 10)
    dist_b = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--dist-batch=")), 2)
    only_ours = "--only-ours" in sys.argv
    b = int(argv[1]) if len(argv) > 1 else 16
    lr = int(argv[2]) if len(argv) > 2 else 48
    sc = int(argv[3]) if len(argv) > 3 else 4
    hu = wu = lr * sc
    dev = torch.device("cuda:0")
    sd = synth.state_dict_for(SHAPES, 123, "liif.")
    params = [torch.from_numpy(sd["imnet." + n]).to(dev).requires_grad_(True) for n in LT.PARAM_NAMES]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)
    n, cells = b * hu * wu, b * lr * lr

    def zero():
        feat.grad = None
        for p in params:
            p.grad = None

    def ours_step():
        zero()
        (LT.LIIFFunction.apply(feat, hu, wu, *params) * r).sum().backward()

    print(f"LIIF decoder  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels, {4 * n} virtual pixels, {cells} cells")
    if only_ours:
        for _ in range(5):
            ours_step()
        torch.cuda.synchronize()
        return

    def eager_step():
        zero()
        (eager_forward(feat, params, (hu, wu)) * r).sum().backward()

    image = LT.image_on_device(params)

    def ours_fwd_nograd():
        from diinn_amd.decoder import liif_decode_features
        with torch.no_grad():
            liif_decode_features(feat.detach(), image, (hu, wu))

    def ours_fwd_grad():
        LT.LIIFFunction.apply(feat, hu, wu, *params)

    for fn in (ours_step, eager_step, ours_fwd_nograd, ours_fwd_grad):
        fn()
        fn()
    t_ours, t_eager, t_f0, t_f1 = [], [], [], []
    for _ in range(runs):
        t_ours.append(once(ours_step))
        t_eager.append(once(eager_step))
        t_f0.append(once(ours_fwd_nograd))
        t_f1.append(once(ours_fwd_grad))
    print(f"  forward, no_grad (P + liif_kernel)                {median(t_f0):8.2f} ms")
    print(f"  forward under grad (P + liif_kernel<SAVE>)        {median(t_f1):8.2f} ms")
    print(f"  step fwd+bwd, HIP path                            {median(t_ours):8.2f} ms   (min {min(t_ours):.2f}, max {max(t_ours):.2f}; {runs} runs)")
    print(f"  step fwd+bwd, reference op sequence (eager)       {median(t_eager):8.2f} ms   (min {min(t_eager):.2f}, max {max(t_eager):.2f})   {median(t_eager) / median(t_ours):.2f}x")
    print(f"  backward = step - forward under grad              {median(t_ours) - median(t_f1):8.2f} ms")

    # the backward's kernels, one group at a time, on buffers of the step's shapes
    lib = N.load()
    feat_c = feat.detach().contiguous()
    _, acts = LT.train_forward(feat_c, image, hu, wu)
    t = LT.virtual_tiles(n)
    vn = 4 * n
    gp = r.permute(1, 0, 2, 3).reshape(3, n).contiguous()
    g = torch.empty((4, t, 256, 32), device=dev)
    geo = LT._geometry(b, lr, lr, hu, wu, dev)
    ks = max(1, min(2 * T.WGRAD_KSPLIT, t))
    rs = max(1, min(T.ROWDOT_SPLITS, t))
    part = torch.empty((3, ks, 256, 257), device=dev)
    part1 = torch.empty((rs, 256, 4), device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plane_gb = t * 256 * 32 * 4 / 1e9

    def k_data():
        N.check(lib.diinn_liif_backward_data(stream, ptr(gp), ptr(acts), ptr(image), ptr(g), b, lr, lr, hu, wu), "diinn_liif_backward_data")

    def k_gemm():
        for li in (3, 2, 1):
            N.check(lib.diinn_plane_gemm_nt(stream, ptr(g[li]), 256, 0, ptr(acts[li - 1]), 256, 0, ptr(part[li - 1]), 256, 256, vn, ks, 1),
                    "diinn_plane_gemm_nt")

    def k_rowdot():
        N.check(lib.diinn_plane_rowdot(stream, ptr(acts[3]), 256, ptr(geo["rhs_t"]), ptr(part1), 256, vn, rs), "diinn_plane_rowdot")
        N.check(lib.diinn_plane_rowdot(stream, ptr(g[0]), 256, ptr(geo["rhs_t"]), ptr(part1), 256, vn, rs), "diinn_plane_rowdot")

    def k_cells():
        LT.cell_sum(g[0], b, lr, lr, hu, wu)

    t_fwd = timed(lambda: LT.train_forward(feat_c, image, hu, wu), runs)
    t_data = timed(k_data, runs)
    t_gemm = timed(k_gemm, runs)
    t_row = timed(k_rowdot, runs)
    t_cell = timed(k_cells, runs)
    flop_chain = 3 * 2.0 * 256 * 256 * vn
    print(f"  diinn_liif_train_fwd (events)                     {t_fwd:8.3f} ms   writes {4 * plane_gb:.2f} GB of planes")
    print(f"  diinn_liif_backward_data (3 kernels)              {t_data:8.3f} ms   {flop_chain / t_data / 1e9:.1f} TFLOP/s, reads+writes {10 * plane_gb:.2f} GB -> {10 * plane_gb / t_data:.2f} TB/s")
    print(f"  3 x diinn_plane_gemm_nt [dW_l | db_l]             {t_gemm:8.3f} ms   {flop_chain / t_gemm / 1e9:.1f} TFLOP/s")
    print(f"  2 x diinn_plane_rowdot (dL; dWc, db0)             {t_row:8.3f} ms   reads {2 * plane_gb:.2f} GB -> {2 * plane_gb / t_row:.2f} TB/s")
    print(f"  diinn_liif_cell_sum                               {t_cell:8.3f} ms   reads {plane_gb:.2f} GB -> {plane_gb / t_cell:.2f} TB/s")
    print(f"  rest of the backward (conv gradients, partial sums, glue)  {median(t_ours) - median(t_f1) - t_data - t_gemm - t_row - t_cell:8.3f} ms")
    print(f"  peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    del acts, g, part, part1

    # gradient distances from float64, given each path's own masks, at a smaller batch
    db = min(dist_b, b)
    f_s = feat.detach()[:db].clone().requires_grad_(True)
    r_s = r[:db].contiguous()
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    ns = db * hu * wu
    img = LT.image_on_device(ps)
    _, acts_s = LT.train_forward(f_s.detach().contiguous(), img, hu, wu)
    saved = LT.saved_activations(acts_s, db, hu, wu)
    masks_ours = [(saved[:, l] > 0).permute(0, 2, 1).contiguous() for l in range(4)]
    del saved, acts_s
    (LT.LIIFFunction.apply(f_s, hu, wu, *ps) * r_s).sum().backward()
    g_ours = [f_s.grad.clone()] + [p.grad.clone() for p in ps]
    f_s.grad = None
    for p in ps:
        p.grad = None
    keep = []
    (eager_forward(f_s, ps, (hu, wu), keep) * r_s).sum().backward()
    g_eager = [f_s.grad.clone()] + [p.grad.clone() for p in ps]
    masks_eager = [torch.stack([keep[v][l].detach() > 0 for v in range(4)]).view(4, ns, 256) for l in range(4)]
    del keep
    p64 = [p.detach().double() for p in ps]
    d_o, g_o = LT.liif_backward_reference(r_s.double(), f_s.detach().double(), p64, (hu, wu), masks=masks_ours)
    d_e, g_e = LT.liif_backward_reference(r_s.double(), f_s.detach().double(), p64, (hu, wu), masks=masks_eager)
    flips = sum(int((a != e).sum()) for a, e in zip(masks_ours, masks_eager))
    print(f"  gradient distances at B={db} ({4 * ns} virtual pixels; {flips} of {4 * 4 * ns * 256} masks differ between the two paths)")
    print("  max|g - float64 given the path's masks| / max|float64|:      HIP path      eager fp32")
    for name, a, e, to, te in zip(["feat"] + LT.PARAM_NAMES, g_ours, g_eager, [d_o] + g_o, [d_e] + g_e):
        print(f"    {name:18s}              {float((a.double() - to).abs().max()) / float(to.abs().max()):10.2e}    "
              f"{float((e.double() - te).abs().max()) / float(te.abs().max()):10.2e}")


if __name__ == "__main__":
    main()
