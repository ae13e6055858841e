"""``pixel_chain_x3_kernel`` on its own (C ABI ``diinn_pixel_chain_x3``): the per-pixel modulation chain of decoder modes 1/2 with
``init_q=True`` in split-bf16 arithmetic, on random pixel records.

Shapes: B = 2, Wu in {9, 17}, rows in {1, 5, 13} -- the ragged edges of the 16 x 8 workgroup and of a wave's 8 x 4 tile, one and
several workgroups.  The yardstick is the chain restated with ``sheets.split_matmul`` in fp32 torch algebra; the bound is
``1e-4 x max|k|`` over the three slots (the fp32 contract's factor on the values the kernel writes).  The two differ by the
summation order of 256 fp32 terms only, a few 1e-7 of max|k|."""
import ctypes as C

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth

gpu = pytest.mark.gpu
HID, PIX_CH = 256, 1280
GUARD = 4096                      # floats behind the records that must stay untouched
CANARY = -77.25
SHAPES = [(2, wu, rows) for wu in (9, 17) for rows in (1, 5, 13)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


_SD = {}


def _weights(mode):
    """(state dict, K_i[:, :256] for i = 1..3, bK_1..3) of a mode-1 or mode-2 decoder with init_q; one per session."""
    if mode not in _SD:
        sd = synth.decoder_state_dict(41, mode=mode, init_q=True)
        kw = [torch.from_numpy(np.asarray(sd[f"K.{i}.0.weight"])).reshape(HID, -1)[:, :HID].contiguous() for i in (1, 2, 3)]
        bk = [torch.from_numpy(np.asarray(sd[f"K.{i}.0.bias"])).reshape(1, HID) for i in (1, 2, 3)]
        _SD[mode] = (sd, kw, bk)
    return _SD[mode]


def _records(b, wu, rows, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((b, rows, wu, PIX_CH), generator=gen, dtype=torch.float32)


def _chain_reference(pix, mode):
    """Slots 1..3 [b, rows, wu, 768] of the fp32 ``split_matmul`` chain on the records ``pix`` (CPU)."""
    from diinn_amd.sheets import split_matmul
    _, kw, bk = _weights(mode)
    flat = pix.reshape(-1, PIX_CH)
    k = torch.relu(flat[:, :HID])
    out = []
    for i in (1, 2, 3):
        seed = bk[i - 1] if mode == 1 else flat[:, HID * i:HID * (i + 1)]
        k = torch.relu(split_matmul(kw[i - 1], k.t()).t() + seed)
        out.append(k)
    return torch.cat(out, 1).reshape(*pix.shape[:3], 3 * HID)


def _run(pix_cpu, packed, bk_seeds, dev):
    """The kernel on a copy of the records with a canary-filled guard behind them; returns (records, guard) on the CPU."""
    import diinn_amd._native as N
    lib = N.load()
    b, rows, wu, _ = pix_cpu.shape
    buf = torch.full((pix_cpu.numel() + GUARD,), CANARY, device=dev)
    buf[:pix_cpu.numel()] = pix_cpu.reshape(-1).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(lib.diinn_pixel_chain_x3(stream, _ptr(buf), _ptr(packed), b, wu, rows, int(bk_seeds)), "diinn_pixel_chain_x3")
    torch.cuda.synchronize()
    got = buf.cpu()
    return got[:pix_cpu.numel()].reshape(pix_cpu.shape), got[pix_cpu.numel():]


def _packed(mode, dev):
    import diinn_amd.decoder as D
    sd, _, _ = _weights(mode)
    return D.pack_state_dict(D.initq_body_state_dict(sd), mode=mode).to(dev)


def test_entry_point_validates_before_it_touches_a_device():
    """diinn_pixel_chain's checks: null pointers, a misaligned ``pix``, empty extents, grid limits; ``bk_seeds`` is any int."""
    import diinn_amd._native as N
    lib = N.load()
    one, odd = C.c_void_p(16), C.c_void_p(8)
    f = lib.diinn_pixel_chain_x3
    assert f(None, None, one, 1, 8, 8, 0) == N.ERR_INVALID_ARG
    assert f(None, one, None, 1, 8, 8, 1) == N.ERR_INVALID_ARG
    assert f(None, odd, one, 1, 8, 8, 0) == N.ERR_INVALID_ARG             # 16-byte seeds
    assert f(None, one, odd, 1, 8, 8, 1) == N.ERR_INVALID_ARG             # 16-byte weight pieces
    for b, wu, rows in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, -3)):
        for bk in (0, 1):
            assert f(None, one, one, b, wu, rows, bk) == N.ERR_INVALID_ARG
    assert f(None, one, one, 70000, 8, 8, 0) == N.ERR_TOO_LARGE
    assert f(None, one, one, 1, 8, 8 * 65536, 1) == N.ERR_TOO_LARGE


@gpu
@pytest.mark.parametrize("bk_seeds", [0, 1])
@pytest.mark.parametrize("b,wu,rows", SHAPES)
def test_chain_on_random_records(dev, b, wu, rows, bk_seeds):
    """Slots 1..3 within 1e-4 x max|k| of the fp32 split_matmul chain; channels 0..255 and 1024..1279 and the guard behind the
    buffer bitwise untouched; the rows split into two launches give the bits of one launch."""
    mode = 1 if bk_seeds else 2
    packed = _packed(mode, dev)
    pix = _records(b, wu, rows, 1000 * wu + rows)
    got, guard = _run(pix, packed, bk_seeds, dev)
    want = _chain_reference(pix, mode)
    scale = float(want.abs().max())
    err = float((got[..., HID:4 * HID] - want).abs().max())
    print(f"bk_seeds {bk_seeds} B {b} Wu {wu} rows {rows}: max|kernel - sheet| = {err:.3e}, max|k| = {scale:.3e}, bound {1e-4 * scale:.3e}")
    assert scale > 0.05 and bool(torch.isfinite(got).all())
    assert err <= 1e-4 * scale
    assert torch.equal(got[..., :HID].view(torch.int32), pix[..., :HID].view(torch.int32))
    assert torch.equal(got[..., 4 * HID:].view(torch.int32), pix[..., 4 * HID:].view(torch.int32))
    assert bool((guard == CANARY).all())
    if rows > 1:                                                   # two launches over [0, cut) and [cut, rows): the same bits
        cut = 1 if rows == 5 else 8
        top, g0 = _run(pix[:, :cut].contiguous(), packed, bk_seeds, dev)
        bot, g1 = _run(pix[:, cut:].contiguous(), packed, bk_seeds, dev)
        assert torch.equal(torch.cat([top, bot], 1).view(torch.int32), got.view(torch.int32))
        assert bool((g0 == CANARY).all()) and bool((g1 == CANARY).all())


@gpu
def test_mode1_seeds_ignore_the_slots_and_a_body_image_without_its_word_answers_nan(dev):
    """``bk_seeds = 1`` never reads slots 1..3: NaN there changes no bit.  A body image without its derived sections' validity word
    (section WLX is one of them) gives NaN in every slot, like the other split-bf16 kernels."""
    import diinn_amd._native as N
    lib = N.load()
    packed = _packed(1, dev)
    pix = _records(2, 9, 5, 7)
    got, _ = _run(pix, packed, 1, dev)
    poisoned = pix.clone()
    poisoned[..., HID:4 * HID] = float("nan")
    again, _ = _run(poisoned, packed, 1, dev)
    assert torch.equal(again[..., HID:4 * HID].view(torch.int32), got[..., HID:4 * HID].view(torch.int32))
    off, size = C.c_size_t(), C.c_size_t()
    assert lib.diinn_packed_section(6, C.byref(off), C.byref(size)) == 0
    bad = packed.clone()
    bad[off.value + 3] = 0.0
    for bk, image in ((1, bad), (0, bad)):
        out, _ = _run(pix, image, bk, dev)
        assert bool(torch.isnan(out[..., HID:4 * HID]).all())
        assert torch.equal(out[..., :HID].view(torch.int32), pix[..., :HID].view(torch.int32))
