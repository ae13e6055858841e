#!/usr/bin/env python3
"""What the decode entry points of the C ABI refuse, and in which order, as a recording: every entry point is called with
never-dereferenced fake pointers (4096; 4104 where an alignment is checked) and a null stream, once per check that it makes and
once per pair of adjacent checks, and the status it returns is stored.  Runs on the CPU in a second (needs the built library).

An entry point is described by its parameter list and by its checks IN THE ORDER IT MAKES THEM; each check is a list of faults, a
fault is a change to the arguments of a good call (``GOOD``).  ``rows()`` gives one row per fault and, for every two adjacent checks,
one row with the first fault of both: the status of that row says which of the two the entry point looks at first.

Only refusals are recorded.  A row whose status is 0 (ok) or 3 (a HIP call failed) passed validation and tried to launch on the fake
pointers: ``record()`` raises on it instead of writing it, so a check that an entry point makes only AFTER its first launch (the
sine mode of ``diinn_decode``, which launches the hoisted conv first, for one) has no row here, and an entry point lists only
the checks in front of its first launch.  ``tests/test_entry_refusals.py`` replays the stored rows and ``record()``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_entry_refusals.py
"""
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import diinn_amd._native as N  # noqa: E402

PATH = os.path.join(HERE, "entry_refusals.json")
FAKE, MISALIGNED = 4096, 4104

# a good call: x2 of a 16 x 16 map, every window the full buffer, the tile the whole image in a contiguous [B,3,32,32]
GOOD = dict(B=1, H=16, W=16, Hu=32, Wu=32, y0=0, y1=32, x0=0, x1=32, r0=0, r1=16, rows=32, sin_mode=2, compute=0, bk_seeds=0,
            feat_row0=0, feat_rows=16, p_row0=0, p_rows=16, out_row0=0, out_rows=32,
            out_row_stride=32, out_plane_stride=32 * 32, out_batch_stride=3 * 32 * 32)
GEOM = "B H W Hu Wu y0 y1 sin_mode".split()

# ---- faults: name -> changes of the arguments ---------------------------------------------------------------------------------
TALL8 = 8 * 65535 + 1          # rows that need 65,536 blocks of 8 (every decode / planes / chain kernel)
TALL4 = 4 * 65535 + 1          # ... of 4 (mode 4's gather)
FAULTS = {
    "B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "Hu=0": dict(Hu=0), "Wu=0": dict(Wu=0),
    "B=65536": dict(B=65536), "H=65536": dict(H=65536, r1=65536, feat_rows=65536, p_rows=65536),
    "y0<0": dict(y0=-1), "y1>Hu": dict(y1=33), "y0==y1": dict(y0=5, y1=5),
    "x0<0": dict(x0=-1), "x1>Wu": dict(x1=33), "x0==x1": dict(x0=5, x1=5),
    "r0<0": dict(r0=-1), "r1>H": dict(r1=17), "r0==r1": dict(r0=5, r1=5),
    "rows=0": dict(rows=0),
    "Hu=1": dict(Hu=1, y1=1, out_rows=1), "Wu=1": dict(Wu=1),
    "extent": dict(Hu=46341, Wu=46341), "extent rows": dict(rows=46341, Wu=46341),
    "sin_mode=-1": dict(sin_mode=-1), "sin_mode=3": dict(sin_mode=3),
    "compute=-1": dict(compute=-1), "compute=5": dict(compute=5),
    "grid.y of 8 rows": dict(Hu=TALL8, Wu=2, y1=TALL8, x1=2, out_rows=TALL8, rows=TALL8, out_row_stride=2,
                             out_plane_stride=2 * TALL8, out_batch_stride=6 * TALL8),
    "grid.y of 4 rows": dict(Hu=TALL4, Wu=2, y1=TALL4, out_rows=TALL4),
    "npix": dict(B=2, Hu=32768, Wu=32768),
    # windows: [row0, row0 + rows) inside the tensor and around what the launch touches
    "feat window row0<0": dict(feat_row0=-1), "feat window rows=0": dict(feat_rows=0), "feat window past H": dict(feat_row0=1),
    "feat window without the rows": dict(feat_row0=8, feat_rows=8),
    "P window row0<0": dict(p_row0=-1), "P window rows=0": dict(p_rows=0), "P window past H": dict(p_row0=1),
    "P window without the rows": dict(p_row0=8, p_rows=8),
    "out window row0<0": dict(out_row0=-1), "out window rows=0": dict(out_rows=0), "out window past Hu": dict(out_row0=1),
    "out window without the rows": dict(out_row0=16, out_rows=16),
    # the tile's strides: a row holds its columns, a plane its rows, a batch item its three planes, below 2^40 floats
    "row stride short": dict(out_row_stride=31), "plane stride short": dict(out_plane_stride=32 * 32 - 1),
    "batch stride short": dict(out_batch_stride=3 * 32 * 32 - 1), "batch stride 2^40+1": dict(out_batch_stride=(1 << 40) + 1),
}


def null(p):
    return p + "=NULL"


def odd(p):
    return p + " misaligned"


def fault(name):
    if name.endswith("=NULL"):
        return {name[:-5]: 0}
    if name.endswith(" misaligned"):
        return {name[:-11]: MISALIGNED}
    return FAULTS[name]


# ---- checks shared by many entry points (each a list of checks, a check a list of fault names) --------------------------------
DIMS = [["B=0", "H=0", "W=0"], ["B=65536", "H=65536"]]
BAND = [["y0==y1", "y0<0", "y1>Hu", "Hu=0", "Wu=0"]]
EXTENT, SIN, COMPUTE = [["extent"]], [["sin_mode=3", "sin_mode=-1"]], [["compute=5", "compute=-1"]]
GRID8, GRID4 = [["grid.y of 8 rows"]], [["grid.y of 4 rows"]]
MODE4_ROWS = [["Wu=1", "Hu=1"], ["y0==y1", "y0<0", "y1>Hu"]]
P_WIN = [["P window row0<0", "P window rows=0", "P window past H", "P window without the rows"]]
OUT_WIN = [["out window row0<0", "out window rows=0", "out window past Hu", "out window without the rows"]]
FEAT_WIN = [["feat window row0<0", "feat window rows=0", "feat window past H", "feat window without the rows"]]


def ptrs(*names):
    return [[null(n) for n in names]]


def band_checks(*pointers):       # the common order of a band entry point
    return ptrs(*pointers) + DIMS + BAND + EXTENT + SIN + GRID8


def lr_rows():                    # diinn_lr_rows_for_band in front of everything else
    return [["y0==y1", "y0<0", "y1>Hu", "H=0", "Hu=0", "Wu=0"]]


def launch_p(feat="feat_dev", ws="workspace_dev", windows=()):   # the hoisted conv's own checks: the first launch follows them
    return ptrs(feat, "packed_dev", ws) + [["B=0", "W=0"], ["B=65536", "H=65536"]] + list(windows)


def decode_checks(feat="feat_dev", ws="workspace_dev", windows=(), compute=True):
    return ptrs(ws) + lr_rows() + (COMPUTE if compute else []) + launch_p(feat, ws, windows)


def tile_checks(pointers, first=(), windows=(), strides=()):
    cols = [["x0<0", "x1>Wu", "x0==x1"]] if strides else []
    return (list(first) + COMPUTE + ptrs(*pointers) + DIMS + BAND + cols + EXTENT + list(windows) + list(strides) + SIN + GRID8)


MODE4_BAND = ["P_dev", "packed_dev", "head_dev", "taps_dev", "out_dev"]
INITQ_ALL = ["feat_dev", "packed_dev", "initq_dev", "pix_dev", "out_dev"]
TRAIN = ["P_dev", "packed_dev", "out_dev", "acts_dev"]
INITQ_TRAIN = ["feat_dev", "packed_dev", "train_image_dev", "pix_dev", "out_dev", "acts_dev"]
TRAIN_GEOM = "B H W Hu Wu sin_mode".split()
TRAIN_TAIL = DIMS + [["Hu=0", "Wu=0"]] + SIN + EXTENT + [["npix"]]

# ---- the entry points: name -> (parameters after the stream, checks in order) -------------------------------------------------
ENTRIES = {
    "diinn_decode": (["feat_dev", "packed_dev", "workspace_dev", "out_dev"] + GEOM, decode_checks(compute=False)),
    "diinn_decode_ex": (["feat_dev", "packed_dev", "workspace_dev", "out_dev"] + GEOM + ["compute"], decode_checks()),
    "diinn_decode_win": (["feat_win_dev", "feat_row0", "feat_rows", "packed_dev", "P_win_dev", "p_row0", "p_rows", "out_win_dev",
                          "out_row0", "out_rows"] + GEOM + ["compute"],
                         decode_checks("feat_win_dev", "P_win_dev", FEAT_WIN + P_WIN)),
    "diinn_decode_band": (["P_dev", "packed_dev", "out_dev"] + GEOM,
                          [["Wu=0"]] + ptrs("P_dev", "packed_dev", "out_dev") + DIMS + BAND + EXTENT + SIN + GRID8),
    "diinn_decode_band_ex": (["P_dev", "packed_dev", "out_dev"] + GEOM + ["compute"],
                             tile_checks(["P_dev", "packed_dev", "out_dev"], first=[["Wu=0"]])),
    "diinn_decode_band_win": (["P_win_dev", "p_row0", "p_rows", "packed_dev", "out_win_dev", "out_row0", "out_rows"] + GEOM + ["compute"],
                              tile_checks(["P_win_dev", "packed_dev", "out_win_dev"], first=[["Wu=0"]], windows=P_WIN + OUT_WIN)),
    "diinn_decode_tile_win": (["P_win_dev", "p_row0", "p_rows", "packed_dev", "out_tile_dev", "out_row_stride", "out_plane_stride",
                               "out_batch_stride", "B", "H", "W", "Hu", "Wu", "y0", "y1", "x0", "x1", "sin_mode", "compute"],
                              tile_checks(["P_win_dev", "packed_dev", "out_tile_dev"], windows=P_WIN,
                                          strides=[["row stride short", "plane stride short", "batch stride short",
                                                    "batch stride 2^40+1"]])),
    "diinn_cell_chain": (["P_dev", "packed_dev", "B", "H", "W", "r0", "r1"],
                         ptrs("P_dev", "packed_dev") + DIMS + [["r0<0", "r1>H", "r0==r1"]]),
    "diinn_pixel_chain": (["pix_dev", "packed_dev", "B", "Wu", "rows", "bk_seeds"],
                          ptrs("pix_dev", "packed_dev") + [["B=0", "Wu=0", "rows=0"]] + [[odd("pix_dev"), odd("packed_dev")]]
                          + [["extent rows"]] + [["grid.y of 8 rows", "B=65536"]]),
    "diinn_decode_mode4_band": (MODE4_BAND + GEOM, ptrs(*MODE4_BAND) + DIMS + MODE4_ROWS + EXTENT + SIN + GRID8 + GRID4),
    "diinn_decode_mode4_x3_band": (MODE4_BAND + GEOM, ptrs(*MODE4_BAND) + DIMS + MODE4_ROWS + EXTENT + SIN + GRID8 + GRID4),
    "diinn_decode_mode4": (["feat_dev", "packed_dev", "head_dev", "workspace_dev", "taps_dev", "out_dev"] + GEOM,
                           ptrs("workspace_dev", "head_dev", "taps_dev", "out_dev") + [["Wu=1", "Hu=1"]]
                           + [["y0==y1", "y0<0", "y1>Hu", "H=0"]] + SIN + launch_p()),
    "diinn_decode_mode4_x3": (["feat_dev", "packed_dev", "head_dev", "workspace_dev", "taps_dev", "out_dev"] + GEOM,
                              ptrs("head_dev", "taps_dev") + ptrs("feat_dev", "packed_dev", "workspace_dev", "out_dev") + DIMS + BAND
                              + EXTENT + SIN + [["Wu=1", "Hu=1"]] + GRID8 + GRID4),
    "diinn_decode_qonly_x3_band": (["P_dev", "packed_dev", "out_dev"] + GEOM,
                                   [["Wu=0"]] + ptrs("P_dev", "packed_dev", "out_dev") + DIMS + BAND + EXTENT + SIN + GRID8),
    "diinn_decode_qonly_x3": (["feat_dev", "packed_dev", "workspace_dev", "out_dev"] + GEOM,
                              band_checks("feat_dev", "packed_dev", "workspace_dev", "out_dev")),
    "diinn_initq_planes": (INITQ_ALL[:4] + GEOM, band_checks(*INITQ_ALL[:4])),
    "diinn_initq_planes_m1": (INITQ_ALL[:4] + GEOM, band_checks(*INITQ_ALL[:4])),
    "diinn_initq_planes_x3": (["feat_dev", "packed_dev", "initq_dev", "initq_x3_dev", "pix_dev"] + GEOM,
                              band_checks("feat_dev", "packed_dev", "initq_dev", "initq_x3_dev", "pix_dev")),
    "diinn_decode_initq_band": (["pix_dev", "packed_dev", "out_dev"] + GEOM, band_checks("pix_dev", "packed_dev", "out_dev")),
    "diinn_decode_initq_band_x3": (["pix_dev", "packed_dev", "out_dev"] + GEOM, band_checks("pix_dev", "packed_dev", "out_dev")),
    "diinn_decode_initq_qonly_band": (["pix_dev", "packed_dev", "out_dev"] + GEOM, band_checks("pix_dev", "packed_dev", "out_dev")),
    "diinn_decode_initq": (INITQ_ALL + GEOM, ptrs("out_dev") + band_checks(*INITQ_ALL[:4])),
    "diinn_decode_initq_x3": (["feat_dev", "packed_dev", "initq_dev", "initq_x3_dev", "pix_dev", "out_dev"] + GEOM,
                              ptrs("out_dev") + band_checks("feat_dev", "packed_dev", "initq_dev", "initq_x3_dev", "pix_dev")),
    "diinn_decode_initq_mode1": (INITQ_ALL + GEOM, band_checks(*INITQ_ALL) + [[odd("pix_dev"), odd("packed_dev")]]),
    "diinn_decode_initq_mode2": (INITQ_ALL + GEOM, band_checks(*INITQ_ALL) + [[odd("pix_dev"), odd("packed_dev")]]),
    "diinn_decode_initq_mode4_band": (["pix_dev", "packed_dev", "head_dev", "taps_dev", "out_dev"] + GEOM,
                                      ptrs("pix_dev", "packed_dev", "head_dev", "taps_dev", "out_dev") + DIMS + MODE4_ROWS + EXTENT + SIN
                                      + GRID8 + GRID4),
    "diinn_decode_initq_mode4": (["feat_dev", "packed_dev", "initq_dev", "head_dev", "pix_dev", "taps_dev", "out_dev"] + GEOM,
                                 ptrs("head_dev", "taps_dev") + band_checks(*INITQ_ALL) + [["Wu=1", "Hu=1"]]),
    "diinn_decode_train_fwd": (TRAIN + TRAIN_GEOM, ptrs(*TRAIN) + TRAIN_TAIL),
    "diinn_decode_train_fwd_qonly": (["chain_dev"] + TRAIN[1:] + TRAIN_GEOM, ptrs("chain_dev", *TRAIN[1:]) + TRAIN_TAIL),
    "diinn_decode_train_fwd_x3": (["P_dev", "packed_dev", "split_dev", "out_dev", "acts_dev"] + TRAIN_GEOM,
                                  [[null("split_dev"), odd("split_dev")]] + ptrs(*TRAIN) + TRAIN_TAIL),
    "diinn_decode_initq_train_fwd": (INITQ_TRAIN + TRAIN_GEOM,
                                     ptrs(*INITQ_TRAIN) + TRAIN_TAIL
                                     + [[odd("packed_dev"), odd("train_image_dev"), odd("pix_dev")]] + GRID8),
    "diinn_decode_initq_train_fwd_qonly": (INITQ_TRAIN + TRAIN_GEOM + ["bk_seeds"],
                                           ptrs(*INITQ_TRAIN) + TRAIN_TAIL
                                           + [[odd("packed_dev"), odd("train_image_dev"), odd("pix_dev")]] + GRID8),
    "diinn_decode_launch_info": (["B", "Hu", "Wu", "y0", "y1", "grid_x", "grid_y", "grid_z", "block"],
                                 [["B=0", "Hu=0", "Wu=0", "y0<0", "y1>Hu", "y0==y1"]]),
    "diinn_decode_kernel_info": (["B", "Hu", "Wu", "y0", "y1", "x0", "x1", "compute", "info"],
                                 [[null("info"), "B=0", "Hu=0", "Wu=0", "y0<0", "y1>Hu", "y0==y1", "x0<0", "x1>Wu", "x0==x1"]] + COMPUTE),
}
NO_STREAM = ("diinn_decode_launch_info", "diinn_decode_kernel_info")
OUT_INTS = ("grid_x", "grid_y", "grid_z", "block")


def arguments(name, faults):
    """The argument list of entry point `name` for a good call with `faults` applied, as plain integers (pointers too)."""
    params = ENTRIES[name][0]
    values = dict(GOOD)
    values.update({p: FAKE for p in params if p.endswith("_dev") or p == "info"})
    values.update({p: 0 for p in OUT_INTS})
    for f in faults:
        values.update({k: v for k, v in fault(f).items() if k in params})
    return [values[p] for p in params]


def rows():
    """(entry point, label, arguments) of every row, in recording order."""
    out, seen = [], set()

    def add(name, label, faults):
        if (name, label) not in seen:                            # (a check that an entry point makes twice is one row)
            seen.add((name, label))
            out.append((name, label, arguments(name, faults)))

    for name, (params, checks) in ENTRIES.items():
        for check in checks:
            for f in check:
                add(name, f, [f])
        for a, b in zip(checks, checks[1:]):
            # the first fault of the earlier check with the first of the later one that changes other arguments
            second = [f for f in b if not set(fault(f)) & set(fault(a[0]))]
            if second:
                add(name, a[0] + " + " + second[0], [a[0], second[0]])
    return out


def call(lib, name, args):
    """Status of one call: integers where the signature says void* / int* become pointers of that value."""
    import ctypes as C
    sig = N.SIGNATURES[name][1]
    stream = [] if name in NO_STREAM else [None]
    conv = []
    for a, t in zip(args, sig[len(stream):]):
        if t is C.c_void_p:
            conv.append(C.c_void_p(a) if a else None)
        elif t in (C.c_int, C.c_longlong):
            conv.append(a)
        else:                                                    # int*: NULL, or a real array for the queries to fill
            conv.append((C.c_int * 4)() if a else None)
    assert len(conv) + len(stream) == len(sig), name
    return int(getattr(lib, name)(*stream, *conv))


def record():
    lib = N.load()
    out = []
    for name, label, args in rows():
        status = call(lib, name, args)
        if status in (0, 3):
            raise RuntimeError(f"{name} [{label}] answered {status}: it passed validation and went on to launch; "
                               "only refusals (1, 2, 4) are recorded")
        out.append({"fn": name, "case": label, "args": args, "status": status})
    return out


def dumps(rec) -> str:
    return "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rec) + "\n]\n"


def main():
    text = dumps(record())
    with open(PATH, "w") as f:
        f.write(text)
    print("wrote", PATH, len(json.loads(text)), "rows,", os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
