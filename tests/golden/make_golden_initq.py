#!/usr/bin/env python3
"""init_q fixtures, from the REAL reference (build container only; /root/reference is read-only and never travels):
``ImplicitDecoder(mode=3, init_q=True)`` (diinn.py:48-51,113-115) -- the synthesis input first goes through
``first_layer = Conv2d(3, 576, 1) + sin``, the embedding multiplies the unfolded features of every HR pixel, and ``Q.0``
reads the embedding -- at the shapes where a per-pixel GEMM over 8 x 8 pixel tiles and a chunked decode go wrong: a 1 x 1 map
(all halo), two output rows, an odd batch with ragged tiles, gain 2, down-scaling, a narrow image of more than one chunk of 8
rows (which is also the ATen small-output index path, Hu + Wu <= 128), a gain-3 stress case with several workgroups each way,
and a SIREN-range first layer (``first_layer.0.weight`` x 30: sine arguments of tens of radians).

  out/<case>   ImplicitDecoder(mode=3, init_q=True).forward in fp32 (whole image, bsize=None)
  d64/<case>   float32(ref64 - ref32), ref64 = the same module after ``.double()`` on the same inputs
  meta/<case>  (b, h, w, hu, wu, gain, first_layer gain)

Inputs are regenerated from ``synth`` (seed 123, ``init_q=True``), never stored.  The reference raised at none of the shapes,
so none is dropped; ``bsize=30000`` gives the bits of ``bsize=None`` at all of them (checked below).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_initq.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import diinn_amd.synth as synth  # noqa: E402
from src.models.components.diinn import ImplicitDecoder  # noqa: E402  (the reference)

# (name, B, H, W, Hu, Wu, gain, first_layer gain)
CASES = [
    ("c1x1_2x2", 1, 1, 1, 2, 2, 1.0, 1.0),                      # all halo
    ("row1x9_2x30", 1, 1, 9, 2, 30, 1.0, 1.0),
    ("b3_7x5_23x18", 3, 7, 5, 23, 18, 1.0, 1.0),                # odd batch; ragged tiles
    ("b2_12x10_31x27_gain2", 2, 12, 10, 31, 27, 2.0, 1.0),
    ("down16x12_8x6", 1, 16, 12, 8, 6, 1.0, 1.0),               # down-scaling
    ("small4x3_110x9", 1, 4, 3, 110, 9, 1.0, 1.0),              # more than one chunk of 8 rows, narrow
    ("b2_17x33_40x100_gain3", 2, 17, 33, 40, 100, 3.0, 1.0),    # several workgroups each way; stress
    ("siren_9x14_36x56", 1, 9, 14, 36, 56, 1.0, 30.0),          # sine arguments of tens of radians
]


def state_dict(gain, fgain):
    sd = synth.decoder_state_dict(123, gain, mode=3, init_q=True)
    sd["first_layer.0.weight"] = (sd["first_layer.0.weight"] * np.float32(fgain)).astype(np.float32)
    return sd


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    with torch.no_grad():
        for name, b, h, w, hu, wu, gain, fgain in CASES:
            out[f"meta/{name}"] = np.array([b, h, w, hu, wu, gain, fgain], dtype=np.float64)
            sd = state_dict(gain, fgain)
            feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
            dec = ImplicitDecoder(mode=3, init_q=True)
            dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            dec.eval()
            y32 = dec(feat, [hu, wu]).numpy().astype(np.float32)
            yb = dec(feat, [hu, wu], 30000).numpy()
            assert np.array_equal(y32, yb), name
            y64 = dec.double()(feat.double(), [hu, wu]).numpy()
            out[f"out/{name}"] = y32
            out[f"d64/{name}"] = (y64 - y32.astype(np.float64)).astype(np.float32)
            print(f"init_q {name}: max|ref32 - ref64| = {np.abs(out[f'd64/{name}']).max():.3e}  "
                  f"max|ref| = {np.abs(y32).max():.4f}")
    path = os.path.join(HERE, "diinn_golden_initq.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
