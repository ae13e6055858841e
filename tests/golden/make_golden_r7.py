#!/usr/bin/env python3
"""Round-7 golden vectors ("What's weak" 1): the reference on the maps the SMALL-MAP kernels take.

Runs only in the build container (needs the reference's read-only checkout; never on the GPU box).

conv_t16_kernel / conv1x1_t16_kernel (csrc/diinn_conv_t16.hip) serve every B = 1 map up to about 48 x 48 whose width is a
multiple of 4 -- the reference's own timing protocol (runtime_test.py: 1 x 3 x 48 x 48) among them -- and no fixture made
from the real reference ran through them: diinn_conv_t16_applies is 0 on every map of the earlier files.

  diinn_golden_r7.npz, ``rdn_layer_gain/<seed>/<B>x<H>x<W>``: the reference's RDN encoder (src/models/components/rdn.py:37-105)
      with PER-LAYER gains (synth.layer_gain, as in round 6) on
          1 x 48 x 48   the protocol's map: 3 strips x 16 workgroups of 3 rows
          1 x 60 x 40   a benchmarks.py x8 map: 3 rows per workgroup, the last strip half filled
          1 x 12 x 12   1 row per workgroup, one partly filled strip (stored whole: 9,216 values)
          1 x 36 x 52   W % 16 = 4: the last strip is one 16-byte piece
          4 x 24 x 24   a batch on this kernel
  diinn_golden_r7_e2e.npz, ``diinn/<H>x<W>_<HU>x<WU>``: the real DIINN(mode=3, init_q=False) (src/models/components/diinn.py:8-19)
      end to end at the protocol's geometry, 48 x 48 -> 96 x 96, and at a non-integer scale, 60 x 40 -> 189 x 126.
  (Two files, so that neither committed file exceeds 1 MiB.)

Per case: <= 16,384 sampled outputs in fp32 (``values``: the parity contract) AND from the same model run in float64
(``values64``: the truth the reference itself is some distance from), max |out|, per-channel sums in float64 over the WHOLE
tensor (the unsampled positions count there).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r7.py      (about 20 s of CPU time)
"""
import json
import os
import sys
import time

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import diinn_amd.synth as synth  # noqa: E402
from src.models.components.diinn import DIINN as RefDIINN  # noqa: E402  (the reference)
from src.models.components.rdn import make_rdn as ref_make_rdn  # noqa: E402

NSAMPLES = 16384
ENC_CASES = [(79, 1, 48, 48), (79, 1, 60, 40), (80, 1, 12, 12), (80, 1, 36, 52), (79, 4, 24, 24)]
E2E_CASES = [(1, 48, 48, 96, 96), (1, 60, 40, 189, 126)]


def store(out, key, y, y64, seed):
    idx = np.random.default_rng(seed).choice(y.size, size=min(NSAMPLES, y.size), replace=False).astype(np.int64)
    out[f"{key}/values"] = y.reshape(-1)[idx].astype(np.float32)
    out[f"{key}/values64"] = y64.reshape(-1)[idx].astype(np.float64)
    out[f"{key}/absmax"] = np.float32(np.abs(y).max())
    out[f"{key}/channel_sums"] = y.astype(np.float64).sum(axis=(0, 2, 3))


def main():
    torch.manual_seed(0)
    with torch.no_grad():
        out = {}
        enc = ref_make_rdn().eval()
        shapes = {k: list(v.shape) for k, v in enc.state_dict().items()}
        out["rdn/shapes_json"] = np.array(json.dumps(shapes))
        for (gseed, b, h, w) in ENC_CASES:
            enc.float()
            sd = synth.state_dict_for(shapes, 123, "enc.", layer_gain_seed=gseed)
            enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            img = torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5))
            t0 = time.time()
            f = enc(img).numpy()
            f64 = enc.double()(img.double()).numpy()
            key = f"rdn_layer_gain/{gseed}/{b}x{h}x{w}"
            store(out, key, f, f64, 1000 * h + w)
            print(f"{key}: {time.time() - t0:.1f} s; max|feat| {np.abs(f).max():.3f}, |ref32 - ref64| {np.abs(f - f64).max():.2e} "
                  f"= {np.abs(f - f64).max() / max(1.0, np.abs(f).max()):.2e} of it", flush=True)
        np.savez(os.path.join(HERE, "diinn_golden_r7.npz"), **out)
        print("wrote", os.path.join(HERE, "diinn_golden_r7.npz"))

        out = {}
        net = RefDIINN(mode=3, init_q=False).eval()
        full = {k: list(v.shape) for k, v in net.state_dict().items()}
        out["diinn/shapes_json"] = np.array(json.dumps(full))
        for (b, h, w, hu, wu) in E2E_CASES:
            net.float()
            net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(full, 123, "diinn.").items()})
            img = torch.from_numpy(synth.uniform(11, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5))
            t0 = time.time()
            y = net(img, [hu, wu], 30000).numpy()
            y64 = net.double()(img.double(), [hu, wu], 30000).numpy()
            key = f"diinn/{h}x{w}_{hu}x{wu}"
            store(out, key, y, y64, 1000 * hu + wu)
            print(f"{key}: {time.time() - t0:.1f} s; max|y| {np.abs(y).max():.4f}, |ref32 - ref64| {np.abs(y - y64).max():.2e}", flush=True)
        np.savez(os.path.join(HERE, "diinn_golden_r7_e2e.npz"), **out)
        print("wrote", os.path.join(HERE, "diinn_golden_r7_e2e.npz"))


if __name__ == "__main__":
    main()
