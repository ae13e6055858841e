#!/usr/bin/env python3
"""Round-9 fixtures, from the REAL reference (build container only; /root/reference is read-only and never travels):
decoder mode 4 (diinn.py:81-90, 140-147) -- mode 3 with last_layer = Conv2d(256, 3, 3, padding=1, padding_mode='reflect')
over the HR grid -- at the shapes where the tap form and the reflect-padded gather go wrong: a 2x2 output (both
reflections land on the same row and the same column), two output rows, two output columns, an odd batch with ragged
tiles, gain 2, down-scaling, the ATen small-output index path (Hu + Wu <= 128) and a gain-3 stress case with more than
one workgroup each way.

  out/mode4/<case>   ImplicitDecoder(mode=4, init_q=False).forward in fp32 (whole image, bsize=None)
  d64/mode4/<case>   float32(ref64 - ref32), ref64 = the same module after ``.double()`` on the same inputs
  meta/<case>        (b, h, w, hu, wu, gain)

Inputs are regenerated from ``synth`` (seed 123), never stored.  The reference raised at none of the eight shapes, so
none is dropped.  (With ``bsize`` set the reference pads every column strip on its own and its result depends on
``bsize``; the fixtures hold ``bsize=None``, the whole-image convolution.)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r9.py
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

# (name, B, H, W, Hu, Wu, gain)
CASES = [
    ("c1x1_2x2", 1, 1, 1, 2, 2, 1.0),                      # both reflections land on the same row and column
    ("row1x9_2x30", 1, 1, 9, 2, 30, 1.0),                  # Hu = 2
    ("col13x3_40x2", 1, 13, 3, 40, 2, 1.0),                # Wu = 2
    ("b3_7x5_23x18", 3, 7, 5, 23, 18, 1.0),                # odd batch; ragged tiles
    ("b2_12x10_31x27_gain2", 2, 12, 10, 31, 27, 2.0),
    ("down16x12_8x6", 1, 16, 12, 8, 6, 1.0),
    ("small4x3_110x9", 1, 4, 3, 110, 9, 1.0),              # Hu + Wu <= 128: ATen's small-output nearest-exact kernel
    ("b2_17x33_40x100_gain3", 2, 17, 33, 40, 100, 3.0),    # more than one workgroup each way; stress
]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    for name, b, h, w, hu, wu, gain in CASES:
        out[f"meta/{name}"] = np.array([b, h, w, hu, wu, gain], dtype=np.float64)
    with torch.no_grad():
        for name, b, h, w, hu, wu, gain in CASES:
            sd = synth.decoder_state_dict(123, gain, mode=4)
            feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
            dec = ImplicitDecoder(mode=4, init_q=False)
            dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            dec.eval()
            y32 = dec(feat, [hu, wu]).numpy().astype(np.float32)
            y64 = dec.double()(feat.double(), [hu, wu]).numpy()
            out[f"out/mode4/{name}"] = y32
            out[f"d64/mode4/{name}"] = (y64 - y32.astype(np.float64)).astype(np.float32)
            print(f"mode 4 {name}: max|ref32 - ref64| = {np.abs(out[f'd64/mode4/{name}']).max():.3e}  "
                  f"max|ref| = {np.abs(y32).max():.4f}")
    path = os.path.join(HERE, "diinn_golden_r9.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
