"""x3_train_time.py [B=16] [LR=48] [scale=4] [--runs=20] [--parent=<libdiinn_hip.so of the parent commit>]
    > profiles/x3_train_times.txt

Mode 3 (init_q=False) under autograd: the fp32 step (training.DecodeMode3Function) against the split-bf16 step
(split_training.DecodeMode3SplitFunction, ImplicitDecoder.hip_autograd_split_bf16) in ONE process, alternating run by run -- the step
times, the forward alone, the two new kernels next to the fp32 kernels they stand in for (diinn_decode_train_fwd_x3 against
diinn_decode_train_fwd, diinn_backward_data_x3 against diinn_backward_data), the device packer, peak memory, and the largest
gradient difference between the two steps (which includes the ReLU gates that fall differently: DESIGN.md 3.7f).
``--only-fp32``: time the fp32 step alone and print one line (run once on this build and once on the parent commit's to show that the
fp32 step did not move)."""
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diinn_amd._native as N  # noqa: E402
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
    sd = synth.decoder_state_dict(123, 1.0)
    params = [torch.from_numpy(sd[k]).to(dev).requires_grad_(True) for k in T.PARAM_NAMES]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hu, wu, device=dev)

    def zero():
        feat.grad = None
        for p in params:
            p.grad = None

    def f32_step():
        zero()
        (T.DecodeMode3Function.apply(feat, hu, wu, N.SIN_DEFAULT, *params) * r).sum().backward()

    if "--only-fp32" in sys.argv:
        for _ in range(3):
            f32_step()
        ts = [once(f32_step) for _ in range(runs)]
        print(f"fp32 step alone  B={b} LR={lr}x{lr} x{sc}: median {median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}; {runs} runs)  library {os.path.relpath(N.LIB_PATH, ROOT)}")
        return

    import diinn_amd.split_training as S
    print(f"mode 3 under autograd, fp32 against split bf16  B={b} LR={lr}x{lr} x{sc} -> {hu}x{wu}: {n} HR pixels; device {torch.cuda.get_device_name(0)}")

    def x3_step():
        zero()
        (S.DecodeMode3SplitFunction.apply(feat, hu, wu, N.SIN_DEFAULT, *params) * r).sum().backward()

    def f32_fwd():
        T.DecodeMode3Function.apply(feat, hu, wu, N.SIN_DEFAULT, *params)

    def x3_fwd():
        S.DecodeMode3SplitFunction.apply(feat, hu, wu, N.SIN_DEFAULT, *params)

    for fn in (f32_step, x3_step, f32_fwd, x3_fwd):
        fn()
        fn()
    f32_step()
    g32 = [feat.grad.clone()] + [p.grad.clone() for p in params]
    x3_step()
    gx3 = [feat.grad.clone()] + [p.grad.clone() for p in params]
    cross = max((float((a - e).abs().max()) / float(e.abs().max()), name) for name, a, e in zip(["feat"] + T.PARAM_NAMES, gx3, g32))
    del g32, gx3
    peaks = []
    for fn in (f32_step, x3_step):
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
    t32, tx3, w32, wx3 = [], [], [], []
    for _ in range(runs):                                         # alternating: a drifting clock meets both alike
        t32.append(once(f32_step))
        tx3.append(once(x3_step))
        w32.append(once(f32_fwd))
        wx3.append(once(x3_fwd))
    print(f"  step fwd+bwd, fp32                       {median(t32):8.2f} ms   (min {min(t32):.2f}, max {max(t32):.2f}; {runs} runs, alternating)")
    print(f"  step fwd+bwd, split bf16                 {median(tx3):8.2f} ms   (min {min(tx3):.2f}, max {max(tx3):.2f})   "
          f"split - fp32 = {median(tx3) - median(t32):+.2f} ms = {100 * (median(tx3) / median(t32) - 1):+.1f} %")
    print(f"  forward under grad, fp32 / split         {median(w32):8.2f} / {median(wx3):.2f} ms")
    print(f"  peak memory: fp32 {peaks[0] / 2**30:.2f} GiB, split {peaks[1] / 2**30:.2f} GiB")
    print(f"  largest max|g_split - g_fp32| / max|g_fp32| over the 19 gradients: {cross[0]:.2e} ({cross[1]}); includes the ReLU gates that "
          f"fall differently in the two forwards")

    # the kernels themselves, on buffers of the step's shapes (event-timed, back to back)
    lib = N.load()
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    det = [p.detach() for p in params]
    feat_c = feat.detach().contiguous()
    out, acts, packed, split = S.train_forward_split(feat_c, det, hu, wu, N.SIN_DEFAULT)
    ws = torch.empty(b * lr * lr * 1024, device=dev)
    t = (n + 31) // 32
    gp = r.permute(1, 0, 2, 3).reshape(3, n).contiguous()
    g = torch.empty((4, t, 512, 32), device=dev)
    q = torch.empty((4, t, 256, 32), device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        N.check(lib.diinn_precompute_P_wpu(stream, ptr(feat_c), ptr(packed), ptr(ws), b, lr, lr, 0, lr), "P")
        k_f32 = timed(lambda: N.check(lib.diinn_decode_train_fwd(stream, ptr(ws), ptr(packed), ptr(out), ptr(acts), b, lr, lr, hu, wu, N.SIN_DEFAULT), "fwd"), runs)
        k_x3 = timed(lambda: N.check(lib.diinn_decode_train_fwd_x3(stream, ptr(ws), ptr(packed), ptr(split), ptr(out), ptr(acts), b, lr, lr, hu, wu, N.SIN_DEFAULT), "fwd x3"), runs)
        b_f32 = timed(lambda: N.check(lib.diinn_backward_data(stream, ptr(gp), ptr(acts), ptr(packed), ptr(g), ptr(q), n), "bwd"), runs)
        b_x3 = timed(lambda: N.check(lib.diinn_backward_data_x3(stream, ptr(gp), ptr(acts), ptr(packed), ptr(split), ptr(g), ptr(q), n), "bwd x3"), runs)
        pk = timed(lambda: N.check(lib.diinn_pack_split_train(stream, ptr(packed), ptr(split)), "pack"), runs)
    gb = n * 8192 / 1e9
    print(f"  diinn_decode_train_fwd    (decode_kernel<SAVE>)            {k_f32:8.3f} ms")
    print(f"  diinn_decode_train_fwd_x3 (decode_bf16x3_kernel<SAVE>)     {k_x3:8.3f} ms   {gb / k_x3 * 1e3:.0f} GB/s of plane writes (8 KiB per pixel)")
    print(f"  diinn_backward_data       (3 x bwd_layer_kernel)           {b_f32:8.3f} ms")
    print(f"  diinn_backward_data_x3    (3 x bwd_layer_x3_kernel)        {b_x3:8.3f} ms")
    print(f"  diinn_pack_split_train    (once per weight version)        {pk:8.3f} ms")


if __name__ == "__main__":
    main()
