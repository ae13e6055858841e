#!/usr/bin/env python3
"""MetaSR decode and training step, direct against hoisted (``MetaSR.hip_hoisted``), on one GPU and one build.

  direct   : diinn_metasr_decode (unfold_cells_kernel + metasr_kernel: the meta-network per HR pixel)
  hoisted  : diinn_precompute_P_wpu (the 3x3 conv [M; B0] per LR cell) + diinn_metasr_decode_hoisted (metasr_hoisted_kernel)

Per geometry, in one process: the two decodes alternate, ``--runs`` samples each, a sample = HIP events around ``--inner`` calls;
then the hoisted path's two entry points alone (events; the new kernel's algorithmic bytes -- 3,084 B of M per cell, 12 B per
pixel -- over its time); then the decoder's training step (forward + backward) with the switch off and on, alternating.  The
margin of a comparison is the slower path's fastest sample over the faster path's slowest one: above 1, the difference exceeds
the run-to-run spread of the alternating runs.

Without arguments every geometry runs in a child process of its own under a time limit, one after the other (the first failure
ends the run), and the report goes to ``--out`` (default profiles/metasr_hoisted_times.txt):
  c2 (B = 1, 256 x 256, x4), and B = 16 of 48 x 48 at x4, x2, x1.5, 62 / 48 = x1.29, x1 and, down-scaling, x0.71, x0.5 and x0.33;
  the report ends with the table of direct / hoisted over pixels per cell and the two geometries between which the paths cross.

usage: metasr_hoisted_time.py [--out=FILE] [--runs=N] [--inner=N]
       metasr_hoisted_time.py --one B LR HR [--runs=N] [--inner=N]          (one geometry, to stdout)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRIES = [("c2", 1, 256, 1024), ("B=16 x4", 16, 48, 192), ("B=16 x2", 16, 48, 96), ("B=16 x1.5", 16, 48, 72),
              ("B=16 x1.29", 16, 48, 62), ("B=16 x1", 16, 48, 48), ("B=16 x0.71", 16, 48, 34), ("B=16 x0.5", 16, 48, 24),
              ("B=16 x0.33", 16, 48, 16)]
CHILD_SECONDS = 240
SHAPES = {"imnet.layers.0.weight": (256, 3), "imnet.layers.0.bias": (256,),
          "imnet.layers.2.weight": (1728, 256), "imnet.layers.2.bias": (1728,)}


def opt(name, default):
    return next((int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")), default)


def stats(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def compare(label, direct, hoisted):
    """One line per path (median, min, max) and the verdict with its margin."""
    (dm, dlo, dhi), (hm, hlo, hhi) = stats(direct), stats(hoisted)
    print(f"  {label}, direct    {dm:8.3f} ms   (min {dlo:.3f}, max {dhi:.3f})")
    print(f"  {label}, hoisted   {hm:8.3f} ms   (min {hlo:.3f}, max {hhi:.3f})   direct / hoisted = {dm / hm:.2f}")
    if hm < dm:
        print(f"    hoisted faster; direct's fastest / hoisted's slowest = {dlo / hhi:.2f}" + ("  (beyond the spread)" if dlo > hhi else "  (WITHIN the spread)"))
    else:
        print(f"    direct faster; hoisted's fastest / direct's slowest = {hlo / dhi:.2f}" + ("  (beyond the spread)" if hlo > dhi else "  (WITHIN the spread)"))
    return dm, hm


def one(b, lr, hr, runs, inner):
    import torch
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.metasr_training as MT
    import diinn_amd.synth as synth
    if not torch.cuda.is_available():
        raise SystemExit("metasr_hoisted_time.py needs a ROCm GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    sd = synth.state_dict_for(SHAPES, 123, "metasr.")
    params = [torch.from_numpy(sd["imnet." + n]).to(dev).requires_grad_(True) for n in MT.PARAM_NAMES]
    feat = torch.from_numpy(synth.encoder_features(123, b, lr, lr)).to(dev).requires_grad_(True)
    r = torch.randn(b, 3, hr, hr, device=dev)
    pixels, cells = b * hr * hr, b * lr * lr
    print(f"MetaSR decoder  B={b} LR={lr}x{lr} -> {hr}x{hr} (x{hr / lr:.2f}): {pixels} HR pixels, {cells} cells, {pixels / cells:.2f} pixels per cell")
    packed, image, _ = MT.images_on_device(params)
    f0 = feat.detach()
    out = torch.empty((b, 3, hr, hr), device=dev)
    ws_u = torch.empty(N.load().diinn_metasr_workspace_bytes(b, lr, lr) // 4, device=dev)
    ws_m = torch.empty(N.load().diinn_workspace_bytes(b, lr, lr) // 4, device=dev)

    def direct():
        D.metasr_decode_features(f0, packed, (hr, hr), out=out, workspace=ws_u)

    def hoisted():
        D.metasr_decode_hoisted(f0, packed, image, (hr, hr), out=out, workspace=ws_m)

    def conv_alone():
        with N.launcher(dev) as run:
            run("diinn_precompute_P_wpu", f0, image, ws_m, b, lr, lr, 0, lr)

    def kernel_alone():
        with N.launcher(dev) as run:
            run("diinn_metasr_decode_hoisted", ws_m, packed, out, b, lr, lr, hr, hr, 0, hr)

    def sample(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    with torch.no_grad():
        direct()
        want = out.clone()
        hoisted()
        torch.cuda.synchronize()
        err = float((out - want).abs().max())
        print(f"  max|hoisted - direct| = {err:.2e} at max|direct| = {float(want.abs().max()):.2f}   (the contract: 1e-4 x max(1, max|ref|) each)")
        for fn in (direct, hoisted, conv_alone, kernel_alone):
            sample(fn, 3)
        t_d, t_h = [], []
        for _ in range(runs):
            t_d.append(sample(direct, inner))
            t_h.append(sample(hoisted, inner))
        dd_, dh_ = compare("decode", t_d, t_h)
        t_c = stats([sample(conv_alone, inner) for _ in range(runs)])
        t_k = stats([sample(kernel_alone, inner) for _ in range(runs)])
        nbytes = cells * 771 * 4 + pixels * 12
        print(f"    diinn_precompute_P_wpu alone        {t_c[0]:8.3f} ms   (min {t_c[1]:.3f}, max {t_c[2]:.3f})")
        print(f"    diinn_metasr_decode_hoisted alone   {t_k[0]:8.3f} ms   (min {t_k[1]:.3f}, max {t_k[2]:.3f})   "
              f"algorithmic bytes {nbytes / 1e6:.1f} MB -> {nbytes / t_k[0] / 1e9:.2f} TB/s")

    def step(fn):
        def run():
            feat.grad = None
            for p in params:
                p.grad = None
            (fn.apply(feat, hr, hr, *params) * r).sum().backward()
        return run

    s_d, s_h = step(MT.MetaSRFunction), step(MT.MetaSRHoistedFunction)
    for fn in (s_d, s_h):
        sample(fn, 2)
    t_d, t_h = [], []
    for _ in range(runs):
        t_d.append(sample(s_d, 1))
        t_h.append(sample(s_h, 1))
    sd_, sh_ = compare("training step fwd+bwd", t_d, t_h)
    print(f"RESULT {pixels / cells:.4f} {dd_:.4f} {dh_:.4f} {sd_:.4f} {sh_:.4f}")


def crossing(rows, col, what):
    """rows: (label, pixels per cell, decode direct, decode hoisted, step direct, step hoisted), by falling pixels per cell."""
    rows = sorted(rows, key=lambda r: -r[1])
    flips = [(a, b) for a, b in zip(rows, rows[1:]) if (a[col] > a[col + 1]) != (b[col] > b[col + 1])]
    if not flips:
        side = "hoisted" if rows[0][col] > rows[0][col + 1] else "direct"
        return f"{what}: {side} is faster at every geometry above (no crossing between {rows[-1][1]:.2f} and {rows[0][1]:.2f} pixels per cell)"
    return "; ".join(f"{what}: the paths cross between {b[1]:.2f} pixels per cell ({b[0]}: direct / hoisted = {b[col] / b[col + 1]:.2f}) and "
                     f"{a[1]:.2f} ({a[0]}: {a[col] / a[col + 1]:.2f})" for a, b in flips)


def main():
    runs, inner = opt("runs", 15), opt("inner", 5)
    if "--one" in sys.argv:
        i = sys.argv.index("--one")
        one(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]), runs, inner)
        return
    out = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles", "metasr_hoisted_times.txt"))
    head = ("# MetaSR decode and training step, direct (metasr_kernel) against hoisted (MetaSR.hip_hoisted): one MI355X, one build, one session\n"
            f"# tools/metasr_hoisted_time.py: per geometry a process of its own; the two paths alternate, {runs} samples each; a decode sample =\n"
            f"# HIP events around {inner} calls, a training sample = one forward + backward of the decoder (weights fixed).  'beyond the spread':\n"
            "# the slower path's fastest sample is slower than the faster path's slowest one.\n\n")
    with open(out, "w") as f:
        f.write(head)
    print(head, end="")
    rows = []
    for label, b, lr, hr in GEOMETRIES:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(b), str(lr), str(hr), f"--runs={runs}", f"--inner={inner}"]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{label}: no result within {CHILD_SECONDS} s; nothing further is started")
        body = [ln for ln in res.stdout.splitlines() if not ln.startswith("RESULT ")]
        for ln in res.stdout.splitlines():
            if ln.startswith("RESULT "):
                rows.append((label, *[float(v) for v in ln.split()[1:]]))
        text = f"## {label}\n" + "\n".join(body) + "\n\n"
        print(text, end="", flush=True)
        with open(out, "a") as f:
            f.write(text)
        if res.returncode != 0:
            print(res.stderr[-3000:])
            raise SystemExit(f"{label}: exit status {res.returncode}; nothing further is started")
    small = [r for r in rows if r[0] != "c2"]                      # one LR size and batch: the scale alone varies
    text = "## direct / hoisted over pixels per cell (medians)\n  geometry      pixels per cell    decode    training step\n"
    for r in rows:
        text += f"  {r[0]:12s}  {r[1]:15.2f}  {r[2] / r[3]:8.2f}  {r[4] / r[5]:15.2f}\n"
    text += crossing(small, 2, "decode") + "\n" + crossing(small, 4, "training step") + "\n"
    print(text, end="")
    with open(out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
