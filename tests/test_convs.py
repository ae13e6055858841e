"""convs.py: the facts about the encoder's 64-output convolutions that the training paths share.

CPU: the form rule (``conv_form``; expectations from the record at ``diinn_rdn_forward_ex``) at default knobs and under knobs, with
``encoder_training.choose_form`` agreeing; ``training._fill_wpu`` on CPU tensors against the host packer's section 13; the counter
constant against include/diinn_hip.h.  GPU: ``training._conv_grads_native`` follows the knobs and launches that form's kernel."""
import ctypes as C
import os
import re

import pytest
import torch

import diinn_amd.synth as synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT_FORMS = [((1, 90, 91), "ksplit"), ((2, 64, 63), "ksplit"),                       # below 8192 pixels
                 ((1, 64, 128), "wino"), ((1, 96, 96), "wino"), ((1, 104, 80), "wino"),   # F(2x2) does them in one round of halves
                 ((1, 100, 148), "wino4"), ((1, 153, 102), "wino4")]


def test_form_rule_at_default_knobs(knobs):
    import diinn_amd.convs as CV
    import diinn_amd.encoder_training as ET
    knobs("DIINN_DEBUG_NCU", 256)                                # the rule's round counts depend on the CU count
    for shape, form in DEFAULT_FORMS:
        assert CV.conv_form(*shape) == form, shape
        assert ET.choose_form(*shape) == form, shape


def test_form_rule_under_knobs(knobs):
    import diinn_amd.convs as CV
    import diinn_amd.encoder_training as ET
    knobs("DIINN_DEBUG_NCU", 256)
    assert CV.conv_form(1, 7, 5) == ET.choose_form(1, 7, 5) == "ksplit"
    knobs("DIINN_ENC_WINO_MIN", 1)
    assert CV.conv_form(1, 7, 5) == ET.choose_form(1, 7, 5) == "wino"
    knobs("DIINN_ENC_WINO4_MIN", 0)
    assert CV.conv_form(1, 7, 5) == ET.choose_form(1, 7, 5) == "wino4"


@pytest.mark.parametrize("seed,gain,mode", [(5, 1.0, 3), (5, 3.0, 3), (123, 1.0, 1), (123, 3.0, 1), (123, 1.0, 2)])
def test_fill_wpu_on_cpu_is_the_host_packers_section_13(seed, gain, mode):
    """Section 13 and the validity word of a training image, bit for bit the host packer's section 13 -- weight layouts 3 and 1
    (the GPU assertion of test_training.py::test_fused_backward_equals_formula_backward_on_gpu, on CPU tensors)."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.training as T
    sd = synth.decoder_state_dict(seed, gain, mode=mode)
    host = D.pack_state_dict(sd, mode=mode)
    packed = torch.zeros_like(host)
    T._fill_wpu(packed, [torch.from_numpy(sd[n]) for n in T.PARAM_NAMES], mode)
    o13, z13 = T._section(13)
    assert z13 == 1024 * 64 * 16 and bool(host[o13:o13 + z13].any())
    assert torch.equal(packed[o13:o13 + z13].view(torch.int32), host[o13:o13 + z13].view(torch.int32))
    word = T._section(6)[0] + 3
    assert packed[word:word + 1].view(torch.int32).item() == N.PACKED_MAGIC_WPU
    rest = torch.ones(packed.numel(), dtype=torch.bool)
    rest[o13:o13 + z13] = False
    rest[word] = False
    assert not bool(packed[rest].any())                          # nothing else is written


def test_counter_constant_is_the_headers():
    import diinn_amd.convs as CV
    with open(os.path.join(ROOT, "include", "diinn_hip.h")) as f:
        (nbytes,) = re.findall(r"^#define\s+DIINN_WINO4_COUNTER_BYTES\s+(\d+)", f.read(), re.M)
    assert CV.WINO4_COUNTER_WORDS * 4 == int(nbytes)


def _direct(form, dp, pk, b, h, w):
    """d_feat from that form's single-layer entry point, called here: a 1024 -> 64 3x3 layer with a zero bias."""
    import diinn_amd._native as N
    import diinn_amd.convs as CV
    lib = N.load()
    dev = dp.device
    out = torch.full((b, 64, h, w), float("nan"), device=dev)
    zero = torch.zeros(64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if form == "wino4":
        ws = CV.w4_area(dev)
        ws[:CV.WINO4_COUNTER_WORDS].zero_()
        N.check(lib.diinn_conv_wino4_ws(stream, ptr(dp), 1024 * h * w, 1024, ptr(pk), ptr(zero), None, 0, ptr(out), 64 * h * w, 0,
                                        b, h, w, ptr(ws), ws.numel()), "diinn_conv_wino4_ws")
    elif form == "wino":
        N.check(lib.diinn_conv_wino(stream, ptr(dp), 1024 * h * w, 1024, ptr(pk), ptr(zero), None, 0, ptr(out), 64 * h * w, 0,
                                    b, h, w), "diinn_conv_wino")
    else:
        N.check(lib.diinn_conv_ksplit(stream, ptr(dp), 1024 * h * w, 1024, 9, ptr(pk), ptr(zero), None, 0, ptr(out), 64 * h * w,
                                      None, 0, 0, b, h, w), "diinn_conv_ksplit")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,w", [(1, 6, 5), (2, 7, 9)])
def test_conv_grads_native_follows_the_knobs(knobs, b, h, w):
    """``_conv_grads_native``'s input gradient is the kernel family the knobs select, on ragged maps smaller than any kernel's tile:
    bit-equal to a direct call of that form's entry point on ``pack_conv3x3`` of the transposed, flipped weight (same kernel, same
    image, same inputs).  Accuracy: test_training.py::test_hoisted_conv_gradients_on_the_library_kernels."""
    import diinn_amd.convs as CV
    import diinn_amd.modules as M
    import diinn_amd.training as T
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(100 * h + w)
    feat = torch.randn(b, 64, h, w, generator=gen).to(dev)
    wx = (torch.randn(1024, 64, 3, 3, generator=gen) * 0.05).to(dev)
    dp = torch.randn(b, 1024, h, w, generator=gen).to(dev)
    wt = wx.flip(2, 3).permute(1, 0, 2, 3).contiguous()
    for form, settings in (("ksplit", ()), ("wino", (("DIINN_ENC_WINO_MIN", 1),)),
                           ("wino4", (("DIINN_ENC_WINO_MIN", 1), ("DIINN_ENC_WINO4_MIN", 0)))):
        for name, value in settings:
            knobs(name, value)
        assert CV.conv_form(b, h, w) == form
        d_wx, d_feat = T._conv_grads_native(feat, wx, dp, True, want_weight=False)
        want = _direct(form, dp, CV.pack_conv3x3(wt, form), b, h, w)
        torch.cuda.synchronize()
        assert d_wx is None and bool(torch.isfinite(d_feat).all())
        assert torch.equal(d_feat, want), form
    assert M.RDN.handoff_status() == 0
