"""Decode step time (hoisted conv P + per-pixel kernels) of decoder mode 3 or mode 4 at the BASELINE geometries c1 (48x48 x2)
and c2 (256x256 x4) on ONE GPU, device events around ``--iters`` calls after a warm-up, ``--rounds`` times each.

    python tools/mode4_time.py --mode 3            # decode_features: diinn_decode_ex
    python tools/mode4_time.py --mode 3 --throughput   # the same on decode_kernel, whatever the launch would choose
    python tools/mode4_time.py --mode 4            # decode_features (one call, whole image) and ImplicitDecoder.forward (row chunks)

``--mode 3`` uses nothing mode 4 added, so the same file times an older checkout of the package when it is put next to it
(profiles/mode4_step_times.txt: the parent commit's mode 3 against this commit's mode 3 and mode 4, alternated in one session)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.synth as synth  # noqa: E402

CONFIGS = [("c1  48x48 x2", 48, 48, 96, 96), ("c2  256x256 x4", 256, 256, 1024, 1024)]


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=int, default=4, choices=(3, 4))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--throughput", action="store_true",
                    help="mode 3: force decode_kernel (DIINN_F32_KERNEL = 1), the form mode 4 has, instead of the launch's own choice")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    if a.throughput:
        import diinn_amd._native as N
        N.debug_set("DIINN_F32_KERNEL", 1)
    sd = synth.decoder_state_dict(123, mode=a.mode)
    packed = D.pack_state_dict(sd, mode=a.mode).to(dev)
    for name, h, w, hu, wu in CONFIGS:
        feat = torch.from_numpy(synth.encoder_features(123, 1, h, w)).to(dev)
        ws = torch.empty(h * w * 1024, device=dev)
        out = torch.empty(1, 3, hu, wu, device=dev)
        iters = a.iters * (10 if hu * wu < 1e5 else 1)
        runs = {}
        if a.mode == 3:
            runs["decode_features"] = lambda: D.decode_features(feat, packed, (hu, wu), out=out, workspace=ws)
        else:
            head = D.pack_head3x3(sd).to(dev)
            taps = torch.empty(hu * wu * 28, device=dev)
            dec = D.ImplicitDecoder(mode=4, init_q=False).to(dev).eval()
            dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            runs["decode_features"] = lambda: D.decode_features(feat, packed, (hu, wu), out=out, workspace=ws, mode=4,
                                                                head=head, taps=taps)

            def fwd():
                with torch.no_grad():
                    return dec(feat, (hu, wu))
            runs[f"forward (chunks of {dec.MODE4_CHUNK_ROWS} rows)"] = fwd
        for what, fn in runs.items():
            ms = [timed(fn, iters) for _ in range(a.rounds)]
            print(f"{a.tag}mode {a.mode}  {name:16s} {what:30s} " + "  ".join(f"{m:8.4f}" for m in ms) +
                  f"  ms   min {min(ms):8.4f}", flush=True)


if __name__ == "__main__":
    main()
