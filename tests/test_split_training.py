"""Mode 3 under autograd in split-bf16 arithmetic (ImplicitDecoder.hip_autograd_split_bf16): the CPU half.

  * the host packer of the split training image (diinn_pack_split_train_host): a permutation with an exact hi/lo pair, the
    modulation pieces of the forward half bit-identical to section 14 (WLX) of diinn_pack_weights, hi/lo as round-to-nearest-even;
  * the emulation sheet (split_training.split_forward_reference / split_chain_backward_reference) against the float64 oracle on
    both cases of tests/golden/diinn_golden_grad.npz -- output, planes, the gradients with the gates PINNED (float64 formulas on
    the emulation's own planes), and the number of ReLU gates that differ from the oracle's fp32 planes;
  * the switch: off, the parent's NotImplementedError text; on, every other variant still refuses.

The end-to-end gradient comparison is deliberately absent here: a modulation pre-activation within the split rounding of zero lands
on the other side of the ReLU kink (2 of 1,548,288 elements in the stress case move K.2.0.weight's gradient by 9 %)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
import diinn_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
HID = 256
SZ_WLX = 3 * 8 * 16 * 4 * 64 * 4                   # floats of one half: [layer 3][m 8][ks 16][piece 4][lane 64][j 8] bf16


def _bf16_rne(x):
    """fp32 array -> its bf16 round-to-nearest-even value, as fp32 (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _pieces(half):
    """One half of the split image, float32 [SZ_WLX] -> bf16 values as fp32 [layer 3][m 8][ks 16][piece 4][lane 64][j 8]."""
    u16 = np.ascontiguousarray(half).view(np.uint16).astype(np.uint32) << 16
    return u16.view(np.float32).reshape(3, 8, 16, 4, 64, 8)


def _chan_of_bf16(ks, h, j):
    return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3)


def _natural(pieces, transposed):
    """[layer][m][ks][piece][lane][j] -> [layer][piece][out 256][in 256] by the layout's own rule (csrc/diinn_layout.h)."""
    out = np.zeros((3, 4, HID, HID), np.float32)
    seen = np.zeros((3, 4, HID, HID), np.int32)
    lane = np.arange(64)
    for m in range(8):
        for ks in range(16):
            for j in range(8):
                a = 32 * m + (lane & 31)
                c = _chan_of_bf16(ks, lane >> 5, j)
                o, i = (c, a) if transposed else (a, c)
                out[:, :, o, i] = pieces[:, m, ks, :, :, j]
                seen[:, :, o, i] += 1
    assert (seen == 1).all()                           # every (out, in) pair exactly once per piece
    return out


@pytest.fixture(scope="module")
def lib():
    import diinn_amd._native as N
    return N.load()


def test_split_image_is_a_permutation_with_an_exact_pair(lib):
    """Weights on a 16-bit grid, (index + 1) * 2^-16 within each 256 x 256 matrix: hi + lo == w exactly, and every weight of WL
    and WLT sits exactly once in its half, at the place the layout names."""
    import diinn_amd.decoder as D
    import diinn_amd.split_training as S
    import diinn_amd.training as T
    assert lib.diinn_split_train_floats() == 2 * SZ_WLX
    grid = ((np.arange(HID * HID, dtype=np.float64) + 1) * 2.0 ** -16).astype(np.float32).reshape(HID, HID)
    sd = {n: np.zeros(T.PARAM_SHAPES[n], np.float32) for n in T.PARAM_NAMES}
    for i in (1, 2, 3):
        sd[f"K.{i}.0.weight"][:, :HID, 0, 0] = grid * 2.0 ** i        # distinct per layer and per branch, still 16 significant bits
        sd[f"Q.{i}.0.weight"][:, :, 0, 0] = grid * 2.0 ** (i + 3)
    split = S.pack_split_host(D.pack_state_dict(sd).numpy())
    for half, transposed in ((split[:SZ_WLX], False), (split[SZ_WLX:], True)):
        nat = _natural(_pieces(half), transposed)
        for i in (1, 2, 3):
            for part, w in ((0, grid * np.float32(2.0 ** i)), (1, grid * np.float32(2.0 ** (i + 3)))):
                hi, lo = nat[i - 1, part], nat[i - 1, part + 2]
                assert np.array_equal(hi + lo, w)                        # exact as a hi/lo pair, every weight in its place
                assert np.array_equal(hi, _bf16_rne(w))


def test_split_image_against_section_14_and_round_to_nearest_even(lib):
    """On synth.decoder_state_dict(123, 1.0): the forward half's modulation pieces are section 14's bit for bit (its synthesis pieces
    differ by the division by 2 pi only); hi == bf16_rne(w) and lo == bf16_rne(w - hi) everywhere in both halves."""
    import diinn_amd.decoder as D
    import diinn_amd.split_training as S
    sd = synth.decoder_state_dict(123, 1.0)
    image = D.pack_state_dict(sd).numpy()
    split = S.pack_split_host(image)
    off, size = C.c_size_t(), C.c_size_t()
    assert lib.diinn_packed_section(14, C.byref(off), C.byref(size)) == 0 and size.value == SZ_WLX
    wlx = image[off.value:off.value + size.value].view(np.uint16).reshape(3, 8, 16, 4, 64, 8)
    fwd = split[:SZ_WLX].view(np.uint16).reshape(3, 8, 16, 4, 64, 8)
    assert np.array_equal(fwd[:, :, :, 0::2], wlx[:, :, :, 0::2])        # k_hi, k_lo
    assert not np.array_equal(fwd[:, :, :, 1::2], wlx[:, :, :, 1::2])    # q_hi, q_lo: radians here, revolutions there
    for half, transposed in ((split[:SZ_WLX], False), (split[SZ_WLX:], True)):
        nat = _natural(_pieces(half), transposed)
        for i in (1, 2, 3):
            for part, w in ((0, sd[f"K.{i}.0.weight"].reshape(HID, -1)[:, :HID]), (1, sd[f"Q.{i}.0.weight"].reshape(HID, HID))):
                hi, lo = nat[i - 1, part], nat[i - 1, part + 2]
                assert np.array_equal(hi, _bf16_rne(w))
                assert np.array_equal(lo, _bf16_rne(w - hi))
    # the synthesis pieces are section 14's without the division: hi of the forward half == bf16_rne of the radians weight (above)
    assert lib.diinn_pack_split_train_host(None, None) != 0


def _cases():
    gold = np.load(os.path.join(HERE, "golden", "diinn_golden_grad.npz"))
    for key in gold.files:
        if key.startswith("meta/"):
            b, h, w, hu, wu, gain = gold[key]
            yield key[5:], int(b), int(h), int(w), int(hu), int(wu), float(gain)


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_emulation_sheet_against_the_float64_oracle(case):
    """Output and planes within the project's contract, 1e-4 * max(1, max|ref|) (measured 4.2e-8 / 8.9e-7 at gain 1, 2.7e-5 / 1.7e-5
    on the stress weights); the gradients of the split chain with the gates pinned -- float64 backward_from_saved on the
    emulation's OWN planes -- within 1e-4 relative per tensor (measured 7.8e-6 / 1.2e-5); ReLU gates of the split layers that differ
    from the oracle's fp32 planes: at most 1e-5 of the 3 * 256 * N elements (measured 0 and 2)."""
    import diinn_amd.split_training as S
    import diinn_amd.training as T
    name, b, h, w, hu, wu, gain = case
    sd = synth.decoder_state_dict(123, gain)
    feat = synth.encoder_features(123, b, h, w)
    r = synth.uniform(123, f"gradw:{name}", (b, 3, hu, wu), 1.0)
    out, acts = S.split_forward_reference(sd, feat, (hu, wu))
    out64, _, _ = orc.reference_gradients(sd, feat, (hu, wu), r, dtype=torch.float64)
    _, acts32 = orc.saved_planes(sd, feat, (hu, wu))
    e_out = float((out.double() - out64).abs().max()) / max(1.0, float(out64.abs().max()))
    e_pl = float((acts - acts32).abs().max()) / max(1.0, float(acts32.abs().max()))
    flips = int(((acts[1:, 0] > 0) != (acts32[1:, 0] > 0)).sum())
    print(f"{name}: out err {e_out:.2e}, planes err {e_pl:.2e}, gates that differ {flips} of {acts[1:, 0].numel()}")
    assert e_out <= 1e-4 and e_pl <= 1e-4
    assert flips <= 1e-5 * acts[1:, 0].numel()
    params = [torch.from_numpy(sd[n]) for n in T.PARAM_NAMES]
    g, f = torch.from_numpy(r), torch.from_numpy(feat)
    d_feat, d_params = S.split_chain_backward_reference(g, f, acts, params, (hu, wu))
    d_feat64, d_params64 = T.backward_from_saved(g, f, acts.double(), params, (hu, wu))
    worst = ("feat", float((d_feat - d_feat64).abs().max()) / float(d_feat64.abs().max()))
    for n, got, ref in zip(T.PARAM_NAMES, d_params, d_params64):
        assert got.shape == ref.shape == tuple(T.PARAM_SHAPES[n])
        e = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
        if e > worst[1]:
            worst = (n, e)
    print(f"{name}: worst pinned gradient {worst[0]} {worst[1]:.2e}")
    assert worst[1] <= 1e-4, worst


PARENT_TEXT = ("diinn_amd: autograd through the HIP decode path covers modes 1-3 in fp32 with init_q=False (mode 3 is the "
               "reference's final model, modes 1/2 its ablations); call mode 4, init_q=True or the bf16 path under "
               "torch.no_grad() (mode 4 in fp32 with init_q=False trains once ImplicitDecoder.hip_autograd_mode4 is set)")


def test_switch_off_refuses_with_the_parents_text():
    import diinn_amd.decoder as D
    dec = D.ImplicitDecoder(mode=3, init_q=False, compute="bf16x3")
    assert dec.hip_autograd_split_bf16 is False and D.ImplicitDecoder.hip_autograd_split_bf16 is False
    x = torch.zeros(1, 64, 2, 2, requires_grad=True)
    with pytest.raises(NotImplementedError) as e:
        dec(x, (4, 4))
    assert str(e.value) == PARENT_TEXT


@pytest.mark.parametrize("kw", [dict(mode=1), dict(mode=2), dict(mode=4), dict(mode=3, init_q=True),
                                dict(mode=3, compute="bf16"), dict(mode=3, compute="bf16_full")],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_switch_on_opens_no_other_variant(kw):
    """Modes 1, 2, 4 and init_q=True with compute="bf16x3", and the other bf16 arithmetics on mode 3, still refuse under autograd."""
    import diinn_amd.decoder as D
    kw = {"init_q": False, "compute": "bf16x3", **kw}
    dec = D.ImplicitDecoder(hip_autograd_split_bf16=True, **kw)
    assert dec.hip_autograd_split_bf16 is True
    x = torch.zeros(1, 64, 2, 2, requires_grad=True)
    with pytest.raises(NotImplementedError) as e:
        dec(x, (4, 4))
    assert str(e.value) == PARENT_TEXT


def test_switch_on_needs_a_gpu_and_fp32_still_trains_the_fp32_way():
    """With the switch on, the mode-3 bf16x3 decoder passes the refusal and reaches the device check (the Function has no CPU form);
    compute="f32" is untouched by the switch: the same device check as without it."""
    import diinn_amd.decoder as D
    x = torch.zeros(1, 64, 2, 2, requires_grad=True)
    for compute in ("bf16x3", "f32"):
        dec = D.ImplicitDecoder(mode=3, init_q=False, compute=compute, hip_autograd_split_bf16=True)
        with pytest.raises(Exception) as e:
            dec(x, (4, 4))
        assert not isinstance(e.value, NotImplementedError)
