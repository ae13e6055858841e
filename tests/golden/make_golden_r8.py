#!/usr/bin/env python3
"""Round-8 fixtures, from the REAL reference (build container only; /root/reference is read-only and never travels):
the decode paths other than mode 3 -- decoder modes 1 and 2 (diinn.py:116-131), LIIF (liif.py:59-127) and MetaSR
(metasr.py:70-104) -- at the shapes where kernels go wrong: a 1x1 map, a 1-row map, a 3-column map, odd batches,
down-scaling, the ATen small-output index path (Hu + Wu <= 128) and a gain-3 stress case.

  out/mode{m}/<case>   ImplicitDecoder(mode=m, init_q=False).forward in fp32 (whole image, bsize=None)
  d64/mode{m}/<case>   float32(ref64 - ref32), ref64 = the same module after ``.double()`` on the same inputs
  out/liif/<case>      LIIF.query_rgb (fp32; the reference cannot run it in float64: grid_sample of its fp32 coordinates
  out/metasr/<case>    MetaSR.query_rgb   against a double feature map raises) on the first six cases
  idx/liif/<n_in>_<n_out>_<v>, rel/liif/...    per-axis tables pulled from the reference's own grid_sample calls, for the
  idx/metasr/<n_in>_<n_out>, rel/metasr/...    (n_in, n_out) pairs of those cases
  meta/<case>          (b, h, w, hu, wu, gain)

Inputs are regenerated from ``synth`` (seed 123), never stored.  Neither comparison decoder raised at any of the six
shapes, the 1x1 map included, so none is dropped.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r8.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import diinn_amd.synth as synth  # noqa: E402
import make_golden_liif as GL  # noqa: E402  (reference_axis_tables: the reference's own arithmetic, shared)
import make_golden_metasr as GM  # noqa: E402
from src.models.components.diinn import ImplicitDecoder  # noqa: E402  (the reference)
from src.models.components.liif import LIIF  # noqa: E402
from src.models.components.metasr import MetaSR  # noqa: E402

# (name, B, H, W, Hu, Wu, gain)
CASES = [
    ("c1x1_5x7", 1, 1, 1, 5, 7, 1.0),
    ("row1x9_4x30", 1, 1, 9, 4, 30, 1.0),
    ("b3_7x5_23x18", 3, 7, 5, 23, 18, 1.0),
    ("b2_12x10_31x27_gain2", 2, 12, 10, 31, 27, 2.0),
    ("col13x3_40x9", 1, 13, 3, 40, 9, 1.0),
    ("down16x12_8x6", 1, 16, 12, 8, 6, 1.0),
    ("small4x3_110x9", 1, 4, 3, 110, 9, 1.0),              # Hu + Wu <= 128: ATen's small-output nearest-exact kernel
    ("b2_17x33_40x100_gain3", 2, 17, 33, 40, 100, 3.0),    # stress: |out| ~ 12
]
N_BASELINE = 6                                             # LIIF / MetaSR run the first six


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    for name, b, h, w, hu, wu, gain in CASES:
        out[f"meta/{name}"] = np.array([b, h, w, hu, wu, gain], dtype=np.float64)
    with torch.no_grad():
        for mode in (1, 2):
            for name, b, h, w, hu, wu, gain in CASES:
                sd = synth.decoder_state_dict(123, gain, mode=mode)
                feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
                dec = ImplicitDecoder(mode=mode, init_q=False)
                dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
                dec.eval()
                y32 = dec(feat, [hu, wu]).numpy().astype(np.float32)
                y64 = dec.double()(feat.double(), [hu, wu]).numpy()
                out[f"out/mode{mode}/{name}"] = y32
                out[f"d64/mode{mode}/{name}"] = (y64 - y32.astype(np.float64)).astype(np.float32)
                print(f"mode {mode} {name}: max|ref32 - ref64| = {np.abs(out[f'd64/mode{mode}/{name}']).max():.3e}  "
                      f"max|ref| = {np.abs(y32).max():.4f}")
        liif, meta = LIIF().eval(), MetaSR().eval()
        lshapes = {k: list(v.shape) for k, v in liif.state_dict().items() if k.startswith("imnet.")}
        mshapes = {k: list(v.shape) for k, v in meta.state_dict().items() if k.startswith("imnet.")}
        pairs = []
        for name, b, h, w, hu, wu, gain in CASES[:N_BASELINE]:
            feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
            for tag, model, shapes in (("liif", liif, lshapes), ("metasr", meta, mshapes)):
                sd = synth.state_dict_for(shapes, 123, tag + ".", gain=gain)
                model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
                coord, cell = model.make_coord_and_cell(feat, (hu, wu))
                y = model.reshape_pred(model.query_rgb(feat, coord, cell), (hu, wu))
                out[f"out/{tag}/{name}"] = y.numpy().astype(np.float32)
                print(f"{tag} {name}: {tuple(y.shape)} max|y| = {float(y.abs().max()):.4f}")
            for pair in ((h, hu), (w, wu)):
                if pair not in pairs:
                    pairs.append(pair)
        for n_in, n_out in pairs:
            for v in (-1, 1):
                idx, rel = GL.reference_axis_tables(liif, n_in, n_out, v)
                out[f"idx/liif/{n_in}_{n_out}_{v}"] = idx
                out[f"rel/liif/{n_in}_{n_out}_{v}"] = rel
            idx, rel = GM.reference_axis_tables(meta, n_in, n_out)
            out[f"idx/metasr/{n_in}_{n_out}"] = idx
            out[f"rel/metasr/{n_in}_{n_out}"] = rel
    path = os.path.join(HERE, "diinn_golden_r8.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
