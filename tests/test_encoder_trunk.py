"""RDN encoder trunk on conv_ksplit_kernel: packing layout on CPU; on the GPU, single
convolutions (both kernel variants) and the whole trunk against the same network on PyTorch-ROCm / MIOpen."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diinn_amd.synth as synth


def test_pack_conv_ksplit_layout():
    import diinn_amd.modules as M
    rng = np.random.default_rng(0)
    for cin, k in ((64, 3), (192, 3), (576, 1)):
        w = torch.from_numpy(rng.standard_normal((64, cin, k, k)).astype(np.float32))
        packed = M.pack_conv_ksplit(w).numpy()
        taps, groups, cw = k * k, cin // 64, cin // 8
        assert packed.size == 64 * cin * taps
        pk = packed.reshape(2, 8, taps, groups, 64, 4)
        for _ in range(300):
            half, wave, tap, g, lane, e = (int(rng.integers(n)) for n in (2, 8, taps, groups, 64, 4))
            co, ch = 32 * half + (lane & 31), wave * cw + 8 * g + 2 * e + (lane >> 5)
            assert pk[half, wave, tap, g, lane, e] == w[co, ch, tap // k, tap % k]
    with pytest.raises(ValueError):
        M.pack_conv_ksplit(torch.zeros(64, 3, 3, 3))


def test_pack_conv_wino_layout():
    """The packed Winograd image holds U = G W G^T (float64 reference) at the documented positions."""
    import diinn_amd.modules as M
    rng = np.random.default_rng(1)
    g = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
    for cin in (8, 64, 192):
        w = rng.standard_normal((64, cin, 3, 3)).astype(np.float32)
        packed = M.pack_conv_wino(torch.from_numpy(w)).numpy()
        assert packed.size == 16 * 64 * cin
        pk = packed.reshape(4, cin // 8, 4, 2, 64, 4)
        u = np.einsum("ia,ocab,jb->ocij", g, w.astype(np.float64), g).astype(np.float32)
        for _ in range(300):
            i, chunk, j, half, lane, e = (int(rng.integers(n)) for n in (4, cin // 8, 4, 2, 64, 4))
            assert pk[i, chunk, j, half, lane, e] == (-1 if j == 2 else 1) * u[32 * half + (lane & 31), 8 * chunk + 2 * e + (lane >> 5), i, j]
    with pytest.raises(ValueError):
        M.pack_conv_wino(torch.zeros(64, 64, 1, 1))


def test_pack_conv_wino4_layout():
    """The packed F(4x4, 3x3) image holds U = G W G^T (float64 reference, 6x6 per pair) at the documented positions."""
    import diinn_amd.modules as M
    rng = np.random.default_rng(2)
    g = np.array(M._WINO4_G, dtype=np.float64)
    for cin in (8, 64, 192):
        w = rng.standard_normal((64, cin, 3, 3)).astype(np.float32)
        packed = M.pack_conv_wino4(torch.from_numpy(w)).numpy()
        assert packed.size == 36 * 64 * cin
        pk = packed.reshape(12, 2, cin // 8, 3, 64, 4)
        u = np.einsum("ia,ocab,jb->ocij", g, w.astype(np.float64), g).astype(np.float32)
        for _ in range(300):
            wave, half, chunk, q, lane, e = (int(rng.integers(n)) for n in (12, 2, cin // 8, 3, 64, 4))
            pos = 3 * wave + q
            want = u[32 * half + (lane & 31), 8 * chunk + 2 * e + (lane >> 5), pos // 6, pos % 6]
            assert abs(pk[wave, half, chunk, q, lane, e] - want) <= 2.4e-7 * abs(want)      # float64 sums in another order: one ulp
    # the transform is exact on a constant filter: F(4x4, 3x3) of an all-ones 3x3 filter sums the patch
    ones = M.pack_conv_wino4(torch.ones(64, 8, 3, 3)).reshape(12, 2, 1, 3, 64, 4)
    gg = g.sum(1)
    assert np.allclose(ones[0, 0, 0, 0, 0, 0].item(), gg[0] * gg[0])
    with pytest.raises(ValueError):
        M.pack_conv_wino4(torch.zeros(64, 64, 1, 1))


WINO_SHAPES = [(1, 64, 48, 48, 1, 0), (2, 320, 13, 21, 1, 0), (1, 512, 5, 3, 0, 1),
               (1, 8, 1, 1, 0, 0), (1, 72, 1, 37, 1, 0), (1, 64, 33, 1, 0, 1),
               (1, 192, 128, 136, 1, 0), (2, 128, 70, 61, 0, 1), (1, 64, 64, 80, 1, 1),
               (1, 576, 31, 50, 1, 0), (1, 64, 256, 240, 1, 1), (1, 128, 250, 255, 0, 0)]


@pytest.mark.gpu
def test_conv_wino4_kernel_matches_fp64_conv():
    """diinn_conv_wino4 (Winograd F(4x4,3x3)): ReLU, residual, strided channel-plane views, odd / ragged maps (partial
    tiles, partial blocks, one-pixel maps, widths that are not multiples of 4: the scalar store path), batch > 1, 8 ..
    576 input channels (1 .. 72 chunks: every phase of the three-slot ring), and more work items than workgroups.
    Bound 2.5e-5 of max|out| on these unit-variance inputs (measured <= 2.0e-5, typically 1e-5: the F(4x4) transforms --
    4 and 5 in B^T, 8 in A^T -- cost a good digit against F(2x2)'s 4e-7; tools/conv_wino4_error.py lists every case).  The
    inputs are seeded and the kernel's sums have a fixed order, so the measured figure reproduces to the bit on every box:
    the 25 % margin covers a different torch build's random stream, nothing else; a larger error is a code change."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(6)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    worst = 0.0
    for (b, cin, h, w, relu, use_res) in WINO_SHAPES + [(1, 16, 40, 44, 0, 0), (1, 24, 17, 36, 1, 1), (1, 32, 16, 32, 0, 0),
                                                         (1, 40, 100, 8, 1, 0), (3, 64, 36, 68, 0, 1)]:
        total = cin + 64
        buf = torch.randn((b, total, h, w), device=dev, generator=gen)          # input = first cin planes of a larger buffer
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out = torch.full((b, 96, h, w), float("nan"), device=dev)
        packed = M.pack_conv_wino4(wt).to(dev)
        st = lib.diinn_conv_wino4(stream, ptr(buf), total * h * w, cin, ptr(packed), ptr(bias),
                                  ptr(res) if use_res else None, 64 * h * w, ptr(out[:, 32:]), 96 * h * w, relu, b, h, w)
        assert st == 0
        torch.cuda.synchronize()
        ref = F.conv2d(buf[:, :cin].double(), wt.double(), bias.double(), padding=1)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out[:, 32:].double() - ref).abs().max())
        scale = max(1.0, float(ref.abs().max()))
        assert err <= 2.5e-5 * scale, (cin, h, w, err)
        worst = max(worst, err / scale)
        assert torch.isnan(out[:, :32]).all()
    print(f"diinn_conv_wino4: worst error {worst:.2e} of max|out|")
    assert lib.diinn_conv_wino4(stream, ptr(buf), 1, 12, ptr(packed), ptr(bias), None, 0, ptr(out), 1, 0, 1, 4, 4) == N.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_conv_wino4_kernel_fuzz():
    """Seeded random shapes (batch 1..3, 8..136 input channels, maps from 1x1 to 70x90, ReLU / residual at random)
    through diinn_conv_wino4 against a float64 convolution."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    rng = np.random.default_rng(12)
    gen = torch.Generator(device=dev).manual_seed(12)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    for _ in range(40):
        b, cin = int(rng.integers(1, 4)), 8 * int(rng.integers(1, 18))
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 91))
        relu, use_res = int(rng.integers(2)), int(rng.integers(2))
        x = torch.randn((b, cin, h, w), device=dev, generator=gen)
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out = torch.full((b, 64, h, w), float("nan"), device=dev)
        packed = M.pack_conv_wino4(wt).to(dev)
        assert lib.diinn_conv_wino4(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), ptr(res) if use_res else None,
                                    64 * h * w, ptr(out), 64 * h * w, relu, b, h, w) == 0
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out.double() - ref).abs().max())
        assert err <= 3e-5 * max(1.0, float(ref.abs().max())), (b, cin, h, w, relu, use_res, err)


@pytest.mark.gpu
def test_conv_wino4_kernel_fuzz_large_maps():
    """Seeded random LARGE shapes (several rounds of workgroups, work items that wrap across tile rows, batch 1..3, widths that
    are / are not multiples of 4) through diinn_conv_wino4 against a float64 convolution."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    rng = np.random.default_rng(21)
    gen = torch.Generator(device=dev).manual_seed(21)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    for _ in range(10):
        b, cin = int(rng.integers(1, 4)), 8 * int(rng.integers(1, 9))
        h, w = int(rng.integers(100, 330)), int(rng.integers(100, 420))
        relu, use_res = int(rng.integers(2)), int(rng.integers(2))
        x = torch.randn((b, cin, h, w), device=dev, generator=gen)
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out = torch.full((b, 64, h, w), float("nan"), device=dev)
        packed = M.pack_conv_wino4(wt).to(dev)
        assert lib.diinn_conv_wino4(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), ptr(res) if use_res else None,
                                    64 * h * w, ptr(out), 64 * h * w, relu, b, h, w) == 0
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out.double() - ref).abs().max())
        assert err <= 3e-5 * max(1.0, float(ref.abs().max())), (b, cin, h, w, relu, use_res, err)


@pytest.mark.gpu
def test_conv_wino4_back_to_back_launches_are_bit_identical():
    """Race screen for the kernel's LDS-DMA / barrier structure: 90 back-to-back launches on the same input (two shapes: one
    workgroup per CU with 64 chunk iterations; ragged, more work items than CUs) all equal the first result bit for bit -- a read
    of staged data in the wrong barrier phase shows up as rare differing tiles, not as a failed tolerance."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(3)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    for (b, cin, h, w) in [(1, 512, 256, 256), (2, 136, 203, 310)]:
        x = torch.rand((b, cin, h, w), device=dev, generator=gen)
        wt = torch.rand((64, cin, 3, 3), device=dev, generator=gen) - 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        packed = M.pack_conv_wino4(wt).to(dev)
        outs = [torch.empty((b, 64, h, w), device=dev) for _ in range(4)]
        for i in range(91):
            assert lib.diinn_conv_wino4(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), None, 0,
                                        ptr(outs[0 if i == 0 else 1 + i % 3]), 64 * h * w, 1, b, h, w) == 0
            if i and i % 3 == 0:
                torch.cuda.synchronize()
                assert all(torch.equal(o, outs[0]) for o in outs[1:]), (cin, h, w, i)


@pytest.mark.gpu
def test_conv_wino4_split_last_round(knobs):
    """diinn_conv_wino4_ws with the last round split over the input channels (forced: DIINN_ENC_WINO4_SPLIT = 2): maps of less
    than one round (every workgroup has part of an item, most of two), of one round and a remainder, ragged widths, batches,
    8 .. 512 input channels (runs of 1 chunk up to 36), ReLU / residual.  Against a float64 convolution at the kernel's own
    bound; against the unsplit launch within 3e-5 of max|out| (the sum over input channels reassociated in the TRANSFORMED
    domain, where either evaluation carries F(4x4)'s ~1e-5: measured 1.8e-5 at 512 channels); 30
    back-to-back launches bit-identical (the parts are added in part order, whoever arrives last); the workspace's counter
    words (tickets, ready counts, the gave-up-waiting mark) all zero afterwards; diinn_conv_wino4_plan says a split happened."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(9)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    wsf = lib.diinn_conv_wino4_workspace_floats()
    ws = torch.zeros(wsf, device=dev)
    info = (C.c_int * 4)()
    nsplit = 0
    for (b, cin, h, w, relu, use_res) in [(1, 512, 192, 192, 1, 0), (1, 64, 100, 100, 0, 1), (1, 8, 64, 64, 1, 0), (1, 136, 97, 203, 1, 1),
                                          (2, 256, 200, 180, 0, 0), (1, 320, 320, 324, 1, 0), (3, 72, 50, 90, 0, 1), (1, 16, 12, 9, 1, 0),
                                          (1, 576, 130, 129, 1, 0)]:
        x = torch.randn((b, cin, h, w), device=dev, generator=gen)
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        packed = M.pack_conv_wino4(wt).to(dev)
        rp = ptr(res) if use_res else None
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        scale = max(1.0, float(ref.abs().max()))
        whole = torch.empty((b, 64, h, w), device=dev)
        assert lib.diinn_conv_wino4(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), rp, 64 * h * w, ptr(whole), 64 * h * w,
                                    relu, b, h, w) == 0
        knobs("DIINN_ENC_WINO4_SPLIT", 2)
        assert lib.diinn_conv_wino4_plan(cin, b, h, w, 1, info) == 0
        nsplit += info[2] > 0
        outs = [torch.full((b, 64, h, w), float("nan"), device=dev) for _ in range(4)]
        for i in range(31):
            assert lib.diinn_conv_wino4_ws(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), rp, 64 * h * w,
                                           ptr(outs[0 if i == 0 else 1 + i % 3]), 64 * h * w, relu, b, h, w, ptr(ws), wsf) == 0
            if i and i % 3 == 0:
                torch.cuda.synchronize()
                assert all(torch.equal(o, outs[0]) for o in outs[1:]), (cin, h, w, i)
        knobs("DIINN_ENC_WINO4_SPLIT", 0)
        off = torch.empty((b, 64, h, w), device=dev)
        assert lib.diinn_conv_wino4_ws(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), rp, 64 * h * w, ptr(off), 64 * h * w,
                                       relu, b, h, w, ptr(ws), wsf) == 0
        assert torch.equal(off, whole)                           # without a split the workspace form IS diinn_conv_wino4
        err = float((outs[0].double() - ref).abs().max())
        assert err <= 2.5e-5 * scale, (cin, h, w, err)
        assert float((outs[0] - whole).abs().max()) <= 3e-5 * scale, (cin, h, w)   # two F(4x4) evaluations, each ~1e-5 from the truth
        if info[2]:
            assert not torch.equal(outs[0], whole), (cin, h, w)   # the split form did run
        assert int(ws[:1024].view(torch.int32).abs().sum()) == 0, (cin, h, w)   # counters back at zero, status word never set
    assert nsplit >= 7
    # argument checks of the workspace form: too small a workspace, a misaligned one
    assert lib.diinn_conv_wino4_ws(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), None, 0, ptr(off), 64 * h * w, 0, b, h, w,
                                   ptr(ws), wsf - 1) == N.ERR_INVALID_ARG
    assert lib.diinn_conv_wino4_ws(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), None, 0, ptr(off), 64 * h * w, 0, b, h, w,
                                   C.c_void_p(ws.data_ptr() + 4), wsf) == N.ERR_INVALID_ARG


@pytest.mark.gpu
def test_conv_wino4_split_handoff_gives_up_loudly(knobs):
    """VERDICT r05 item 3 / ADVICE r05: a last arriver that runs out of patience must not sum whatever is in the slabs.  With
    DIINN_ENC_WINO4_FAULT = 1 the split parts store their slabs but never count them ready (and the wait is short): every output
    of every split item is NaN -- never a plausible number --, items that ran whole are untouched, the workspace's STICKY status
    word is set, a later launch on the same workspace without the fault is poisoned as well (a forward's counter reset does
    not clear the word), and diinn_conv_wino4_ws_status reports and clears it; after that the workspace computes again,
    bit-identical to a fresh one."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(23)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    wsf = lib.diinn_conv_wino4_workspace_floats()
    ws, fresh = torch.zeros(wsf, device=dev), torch.zeros(wsf, device=dev)
    info = (C.c_int * 4)()
    st = C.c_int(-1)
    knobs("DIINN_ENC_WINO4_SPLIT", 2)
    for (b, cin, h, w) in [(1, 256, 192, 192), (1, 512, 320, 324)]:      # less than a round; a whole round + a remainder
        x = torch.randn((b, cin, h, w), device=dev, generator=gen)
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        packed = M.pack_conv_wino4(wt).to(dev)

        def run(workspace):
            out = torch.zeros((b, 64, h, w), device=dev)
            assert lib.diinn_conv_wino4_ws(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), None, 0, ptr(out), 64 * h * w,
                                           1, b, h, w, ptr(workspace), wsf) == 0
            return out
        good = run(fresh)
        assert lib.diinn_conv_wino4_plan(cin, b, h, w, 1, info) == 0 and info[2] > 0
        whole_items = info[1]
        assert lib.diinn_conv_wino4_ws_status(stream, ptr(ws), 0, C.byref(st)) == 0 and st.value == 0
        knobs("DIINN_ENC_WINO4_FAULT", 1)
        bad = run(ws)
        knobs("DIINN_ENC_WINO4_FAULT", 0)
        torch.cuda.synchronize()
        nan = torch.isnan(bad)
        assert bool(nan.any())
        assert bool(torch.equal(bad[~nan], good[~nan]))           # what is not NaN is RIGHT (the whole items), never a stale sum
        # the NaN region is exactly the split items: work items are (block of 128 x 4 pixels in tile order, output half)
        frac = float(nan.float().mean())
        assert abs(frac - (1.0 - whole_items / info[0])) < 0.02, (frac, whole_items, info[0])
        assert int(ws[:512].view(torch.int32).abs().sum()) == 0   # counters were reset even so
        # sticky: the next launch (no fault any more; counters re-zeroed as a forward does) is poisoned too
        ws[:512].zero_()
        again = run(ws)
        assert bool(torch.isnan(again).any()) and bool(torch.equal(torch.isnan(again), nan))
        assert lib.diinn_conv_wino4_ws_status(stream, ptr(ws), 1, C.byref(st)) == 0 and st.value == 1
        assert lib.diinn_conv_wino4_ws_status(stream, ptr(ws), 0, C.byref(st)) == 0 and st.value == 0
        assert bool(torch.equal(run(ws), good))                   # cleared: computes again, bit for bit
    assert lib.diinn_conv_wino4_ws_status(stream, None, 0, C.byref(st)) == N.ERR_INVALID_ARG
    assert lib.diinn_conv_wino4_ws_status(stream, ptr(ws), 0, None) == N.ERR_INVALID_ARG


@pytest.mark.gpu
def test_rdn_handoff_status_is_sticky_across_forwards(knobs):
    """The module keeps ONE split area per (device, stream) across forwards: a give-up in one forward (forced) turns that
    forward's features into NaN, stays visible to RDN.handoff_status() after a SECOND forward (whose counter reset must not
    clear it, and whose features are NaN as well), and clearing re-arms the area."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    net = M.make_rdn().to(dev).eval()
    x = torch.rand(1, 3, 200, 180, device=dev)
    M.RDN.handoff_status(clear=True)
    with torch.no_grad():
        good = net(x)
        assert bool(torch.isfinite(good).all()) and M.RDN.handoff_status(clear=False) == 0
        knobs("DIINN_ENC_WINO4_FAULT", 1)
        bad = net(x)
        knobs("DIINN_ENC_WINO4_FAULT", 0)
        assert bool(torch.isnan(bad).any())
        still = net(x)                                            # no fault now, same area: poisoned until somebody looked
        assert bool(torch.isnan(still).any())
        assert M.RDN.handoff_status(clear=True) == 1 and M.RDN.handoff_status(clear=False) == 0
        assert bool(torch.equal(net(x), good))


@pytest.mark.gpu
def test_trunk_entry_point_takes_uninitialised_buffers():
    """diinn_rdn_forward_ex with planes and a split area full of garbage (every word 0xFFFFFFFF: full arrival counters, slabs),
    the area's status word zeroed as its owner does once: the features of the module's own forward, bit for bit, with the
    algorithm that forward takes -- F(4x4) on a map whose last round splits, F(2x2), the direct sum, and split bf16."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    torch.manual_seed(9)
    enc = M.make_rdn().to(dev).eval()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.diinn_rdn_wino4_applies(1, 200, 180) == 1 and lib.diinn_rdn_wino4_applies(1, 100, 120) == 0
    for (b, h, w, algo) in [(1, 200, 180, N.RDN_ALGO_WINO4), (1, 100, 120, N.RDN_ALGO_WINO), (1, 40, 44, N.RDN_ALGO_DIRECT),
                            (1, 256, 256, N.RDN_ALGO_X3)]:
        x = torch.rand(b, 3, h, w, device=dev)
        enc.hip_split_bf16 = algo == N.RDN_ALGO_X3
        with torch.no_grad():
            want = enc(x)
            sfe1 = enc._sfe1_hip(x)
        enc.hip_split_bf16 = False
        packed, biases = enc._hip_packed(dev)
        wino = enc._hip_packed_wino(dev) if algo in (N.RDN_ALGO_WINO, N.RDN_ALGO_X3) else None
        wino4 = enc._hip_packed_wino4(dev) if algo == N.RDN_ALGO_WINO4 else None
        x3 = enc._hip_packed_x3(dev) if algo == N.RDN_ALGO_X3 else None
        planes = torch.empty(lib.diinn_rdn_planes_floats(algo, b, h, w), dtype=torch.float32, device=dev)
        area = torch.empty(lib.diinn_conv_wino4_workspace_floats(), dtype=torch.float32, device=dev)
        planes.view(torch.int32).fill_(-1)
        area.view(torch.int32).fill_(-1)
        area[512:1024].zero_()                                    # bytes [2048, 4096): the status word (word 1023)
        out = torch.full_like(want, float("nan"))
        st = lib.diinn_rdn_forward_ex(stream, algo, ptr(sfe1), ptr(packed), ptr(wino), ptr(wino4), ptr(x3), ptr(biases),
                                      ptr(planes), ptr(area), ptr(out), b, h, w)
        assert st == 0
        status = C.c_int(1)
        assert lib.diinn_conv_wino4_ws_status(stream, ptr(area), 0, C.byref(status)) == 0 and status.value == 0, (b, h, w)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, want), (b, h, w)
    assert M.RDN.handoff_status(clear=False) == 0


@pytest.mark.gpu
def test_conv_wino4_split_handoff_under_load_and_changing_inputs(knobs):
    """The slab hand-off of the split form, screened the way the guide asks (cdna_hip_programming.md, Guideline 16: "test every
    hand-off under UNEVEN load ... checking every word"): the SAME workspace serves launches on ALTERNATING inputs -- a part
    summed from a stale slab (the previous launch's bytes at the same address, still in some L1 or L2) would reproduce the
    previous input's partial sums, which a repeat on one input can never show -- while a second stream keeps half the chip
    busy with decode launches of changing size, so the parts of an item arrive in changing order.  Every launch must equal,
    bit for bit, the first launch on its input; counters end at zero."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(17)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    wsf = lib.diinn_conv_wino4_workspace_floats()
    ws = torch.zeros(wsf, device=dev)
    knobs("DIINN_ENC_WINO4_SPLIT", 2)
    # background load: decodes of a small map at changing output sizes on a side stream
    packed_dec = D.pack_state_dict(synth.decoder_state_dict(3)).to(dev)
    feat = torch.from_numpy(synth.encoder_features(3, 1, 64, 64)).to(dev)
    side = torch.cuda.Stream(device=dev)
    main = torch.cuda.current_stream(dev)
    for (b, cin, h, w) in [(1, 256, 192, 192), (1, 512, 100, 100), (2, 128, 200, 180)]:
        xs = [torch.randn((b, cin, h, w), device=dev, generator=gen) for _ in range(2)]
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        packed = M.pack_conv_wino4(wt).to(dev)
        first = [None, None]
        stream = C.c_void_p(main.cuda_stream)
        for i in range(24):
            k = i & 1
            if i % 3 == 0:                                       # uneven load: another kernel takes CUs for a while
                with torch.cuda.stream(side):
                    D.decode_features(feat, packed_dec, (96 + 32 * (i % 5), 160))
            out = torch.empty((b, 64, h, w), device=dev)
            assert lib.diinn_conv_wino4_ws(stream, ptr(xs[k]), cin * h * w, cin, ptr(packed), ptr(bias), None, 0, ptr(out), 64 * h * w,
                                           1, b, h, w, ptr(ws), wsf) == 0
            if first[k] is None:
                first[k] = out
            else:
                assert torch.equal(out, first[k]), (cin, h, w, i)
        torch.cuda.synchronize()
        assert not torch.equal(first[0], first[1])
        assert int(ws[:1024].view(torch.int32).abs().sum()) == 0, (cin, h, w)


def test_wino4_split_plan(knobs):
    """diinn_conv_wino4_plan (host only; the compute-unit count fixed at an MI355X's 256 through DIINN_DEBUG_NCU, so the numbers
    below hold on any box: a partitioned part, a 304-CU one, no device at all): whole rounds stay whole, the remainder is cut into
    equal runs over pairs of workgroups (the two output halves of a block side by side), never for a full last round, never
    without a workspace; the cost model leaves thin layers of a half-filled round whole."""
    import ctypes as C
    import diinn_amd._native as N
    lib = N.load()
    info = (C.c_int * 4)()
    knobs("DIINN_DEBUG_NCU", 256)

    def plan(cin, b, h, w, ws=1):
        assert lib.diinn_conv_wino4_plan(cin, b, h, w, ws, info) == 0
        return list(info)
    assert plan(512, 1, 256, 256) == [256, 256, 0, 0]            # exactly one round
    assert plan(512, 1, 192, 192, 0) == [144, 144, 0, 0]         # no workspace, no split
    items, whole, wgs, u = plan(512, 1, 192, 192)
    assert (items, whole, wgs, u) == (144, 0, 256, 39)           # 72 blocks x (64 chunks + 4 overhead units) over 128 pairs
    assert plan(64, 1, 192, 192)[2] == 0                          # 8 chunks: two prologues cost more than the split saves
    items, whole, wgs, u = plan(512, 1, 384, 384)
    assert (items, whole) == (576, 512) and wgs == 256 and u == 17
    assert plan(512, 1, 320, 320)[:2] == [400, 256]
    assert lib.diinn_conv_wino4_plan(12, 1, 8, 8, 1, info) == N.ERR_INVALID_ARG
    # a part with more compute units than the slab area has workgroup slots (304: an MI300X): plan, rounds and dispatch rule
    # all describe the split of the CLIPPED count -- 576 items = 2 rounds of 256 + 64, not 1 of 304 + 272
    knobs("DIINN_DEBUG_NCU", 304)
    items, whole, wgs, u = plan(512, 1, 384, 384)
    assert (items, whole) == (576, 512) and 0 < wgs <= 256
    knobs("DIINN_DEBUG_NCU", 64)                                  # a partitioned part: rounds of 64
    items, whole, wgs, u = plan(512, 1, 192, 200)
    assert items == 150 and whole == 128 and 0 < wgs <= 64


def test_wino4_dispatch_rule(knobs):
    """diinn_rdn_wino4_applies: the F(4x4) kernel where it needs fewer rounds of workgroups (one round = 1.44 F(2x2) rounds
    of whole blocks -- r05: 1.40; a last round filled to r costs 0.27 + 0.86 r of one since round 5: it is split over the input
    channels -- and at least 0.49 of one where it is the map's only round); never on the split-K kernel's small maps;
    DIINN_ENC_WINO4_MIN = n replaces the rule.  Measured on 22 + 32 shapes (profiles/r05_enc_trunk_times.txt): right on all of the
    last table after the refit (176 x 176 moved to F(4x4)) but for 96 x 96, which the refit sent to F(4x4) 15 % behind F(2x2)
    (3.66 against 4.23 ms); measured again with 12 more small maps (profiles/enc_wino4_ab_small_maps.txt): maps that F(2x2) does in
    one round of half blocks (92 .. 96-pixel squares, 64 x 128, 72 x 120, 88 x 96, 104 x 80: 3.5 .. 3.6 against 4.13 .. 4.22 ms) stay
    on F(2x2), maps just above (100 x 148, 102 x 153, 153 x 102: 6.1 .. 6.2 against 4.5 .. 5.0 ms) take F(4x4).
    test_wino4_dispatch_rule_replays_the_measured_tables holds the rule to every row of both files."""
    import diinn_amd._native as N
    lib = N.load()
    knobs("DIINN_DEBUG_NCU", 256)                                 # the table below is an MI355X's
    want = {(1, 256, 256): 1, (1, 512, 512): 1, (1, 224, 224): 1, (1, 192, 192): 1, (1, 384, 384): 1, (1, 240, 256): 1,
            (1, 128, 128): 0, (1, 144, 144): 1, (1, 160, 160): 1, (1, 176, 176): 1, (1, 112, 112): 0, (1, 96, 100): 0, (1, 48, 48): 0, (2, 128, 130): 1,
            (1, 92, 92): 0, (1, 96, 96): 0, (1, 92, 96): 0,  # one thinly filled F(4x4) round (34 .. 36 items) against one round of F(2x2) halves: 3.6 vs 4.15 ms
            (1, 64, 128): 0, (1, 104, 80): 0, (1, 100, 148): 1, (1, 153, 102): 1, (3, 100, 100): 1,
            (1, 270, 480): 1, (1, 320, 180): 1,      # work items are runs of 32 consecutive tiles: the map's width leaves none part empty
            (2, 200, 180): 1,                        # 284 work items = one round and 28 items: split, 12.2 ms (whole 15.6; F(2x2) 14.6)
            (16, 48, 48): 1,                         # the training batch's input gradient (160 items)
            (4, 256, 256): 1, (0, 4, 4): 0}
    for (b, h, w), yes in want.items():
        assert lib.diinn_rdn_wino4_applies(b, h, w) == yes, (b, h, w)
    knobs("DIINN_ENC_WINO4_MIN", 0)
    assert lib.diinn_rdn_wino4_applies(1, 128, 128) == 1 and lib.diinn_rdn_wino4_applies(1, 48, 48) == 0
    knobs("DIINN_ENC_WINO_MIN", 0)
    assert lib.diinn_rdn_wino4_applies(1, 48, 48) == 1
    knobs("DIINN_ENC_WINO4_MIN", 1 << 40)
    assert lib.diinn_rdn_wino4_applies(1, 512, 512) == 0


def _wino4_ab_rows(name):
    """{(B, H, W): (F(2x2) ms, F(4x4) ms)} of a table written by tools/enc_wino4_trunk_ab.py: the LAST measurement of a shape."""
    import os
    import re
    rows = {}
    line_re = re.compile(r"^(\d+(?:x\d+x\d+)?) \(rule: .*?\): F\(2,3\) ([0-9.]+) ms\s+F\(4,3\) ([0-9.]+) ms")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", name)) as f:
        for line in f:
            m = line_re.match(line)
            if m:
                dims = [int(v) for v in m.group(1).split("x")]
                shape = tuple(dims) if len(dims) == 3 else (1, dims[0], dims[0])
                rows[shape] = (float(m.group(2)), float(m.group(3)))
            else:
                assert "F(2,3)" not in line or line.startswith("#"), line          # no measurement is passed over
    return rows


def test_wino4_dispatch_rule_replays_the_measured_tables(knobs):
    """diinn_rdn_wino4_applies against every F(2x2) / F(4x4) A/B measurement on record (an MI355X's 256 compute units forced): the 32
    shapes of profiles/r05_enc_trunk_times.txt and the small maps of profiles/enc_wino4_ab_small_maps.txt (the last measurement of a
    shape counts).  The rule must name the faster form wherever the slower one costs more than 3 % extra -- the rule's own
    hysteresis (it moves to F(4x4) at 0.97 of the F(2x2) estimate); a shape is left unjudged for no other reason, and none of the
    first table's is (its smallest gap: 176 x 176 at 7.6 %)."""
    import diinn_amd._native as N
    lib = N.load()
    knobs("DIINN_DEBUG_NCU", 256)

    def replay(rows):
        judged, close, wrong = 0, [], []
        for (b, h, w), (t2, t4) in sorted(rows.items()):
            if max(t2, t4) <= 1.03 * min(t2, t4):
                close.append((b, h, w))
                continue
            judged += 1
            if lib.diinn_rdn_wino4_applies(b, h, w) != int(t4 < t2):
                wrong.append(((b, h, w), t2, t4))
        return judged, close, wrong

    r05 = _wino4_ab_rows("r05_enc_trunk_times.txt")
    judged, close, wrong = replay(r05)
    print(f"r05_enc_trunk_times.txt: {judged} shapes judged, {len(close)} within 3 %")
    assert wrong == []
    assert len(r05) >= 32 and judged == len(r05) and close == []
    small = _wino4_ab_rows("enc_wino4_ab_small_maps.txt")
    assert len(small) >= 13 and {(1, 92, 92), (1, 96, 96), (1, 64, 128), (1, 100, 148), (1, 153, 102), (1, 128, 96)} <= set(small)
    both = dict(r05)
    both.update(small)                                           # (96 x 96 is in both: the later measurement counts)
    judged, close, wrong = replay(both)
    print(f"both tables: {len(both)} shapes, {judged} judged, within 3 %: {close}")
    assert wrong == []
    assert len(both) >= 44 and judged == len(both) and close == []   # (the smallest gap of the second table: 100 x 100 at 13.8 %)


@pytest.mark.gpu
def test_conv_wino_kernel_matches_fp64_conv():
    """diinn_conv_wino (Winograd F(2x2,3x3)): ReLU, residual, strided channel-plane views, odd / ragged maps (partial
    tiles, partial blocks, one-pixel maps), left / right border blocks and interior blocks, batch > 1."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    for (b, cin, h, w, relu, use_res) in WINO_SHAPES:           # (the last two: >= 448 blocks, both halves per workgroup)
        total = cin + 64
        buf = torch.randn((b, total, h, w), device=dev, generator=gen)          # input = first cin planes of a larger buffer
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out = torch.full((b, 96, h, w), float("nan"), device=dev)
        packed = M.pack_conv_wino(wt).to(dev)
        st = lib.diinn_conv_wino(stream, ptr(buf), total * h * w, cin, ptr(packed), ptr(bias),
                                 ptr(res) if use_res else None, 64 * h * w, ptr(out[:, 32:]), 96 * h * w, relu, b, h, w)
        assert st == 0
        torch.cuda.synchronize()
        ref = F.conv2d(buf[:, :cin].double(), wt.double(), bias.double(), padding=1)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out[:, 32:].double() - ref).abs().max())
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (cin, h, w, err)
        assert torch.isnan(out[:, :32]).all()
    assert lib.diinn_conv_wino(stream, ptr(buf), 1, 12, ptr(packed), ptr(bias), None, 0, ptr(out), 1, 0, 1, 4, 4) == N.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_sfe1_kernel_matches_fp64_conv():
    """diinn_sfe1_forward (SFENet1: 3x3, 1..4 -> 64 channels, zero padding) against a float64 convolution."""
    import ctypes as C
    import diinn_amd._native as N
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(2)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    for (b, cin, h, w) in [(1, 3, 48, 48), (2, 3, 17, 301), (1, 1, 1, 1), (1, 4, 5, 3), (1, 3, 256, 256), (3, 2, 33, 1)]:
        x = torch.randn((b, cin, h, w), device=dev, generator=gen)
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        out = torch.full((b, 64, h, w), float("nan"), device=dev)
        assert lib.diinn_sfe1_forward(stream, ptr(x), cin, ptr(wt), ptr(bias), ptr(out), b, h, w) == 0
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        err = float((out.double() - ref).abs().max())
        assert err <= 5e-6 * max(1.0, float(ref.abs().max())), (b, cin, h, w, err)
    assert lib.diinn_sfe1_forward(stream, ptr(x), 5, ptr(wt), ptr(bias), ptr(out), 1, 4, 4) == N.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_conv_wino_kernel_fuzz():
    """Seeded random shapes (batch 1..3, 8..136 input channels, maps from 1x1 to 70x90, ReLU / residual at random)
    through diinn_conv_wino against a float64 convolution: every border / partial-tile / partial-block combination."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    rng = np.random.default_rng(11)
    gen = torch.Generator(device=dev).manual_seed(11)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    for _ in range(40):
        b, cin = int(rng.integers(1, 4)), 8 * int(rng.integers(1, 18))
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 91))
        relu, use_res = int(rng.integers(2)), int(rng.integers(2))
        x = torch.randn((b, cin, h, w), device=dev, generator=gen)
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out = torch.full((b, 64, h, w), float("nan"), device=dev)
        packed = M.pack_conv_wino(wt).to(dev)
        assert lib.diinn_conv_wino(stream, ptr(x), cin * h * w, cin, ptr(packed), ptr(bias), ptr(res) if use_res else None,
                                   64 * h * w, ptr(out), 64 * h * w, relu, b, h, w) == 0
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out.double() - ref).abs().max())
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (b, cin, h, w, relu, use_res, err)


@pytest.mark.gpu
def test_conv_ksplit_kernel_matches_torch():
    """diinn_conv_ksplit: 3x3 / 1x1, ReLU, residual, two destinations, strided channel-plane views, ragged maps."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    for (b, cin, k, h, w, relu, use_res, two) in [(1, 64, 3, 48, 48, 1, 0, 0), (2, 320, 3, 13, 21, 1, 0, 1),
                                                  (1, 576, 1, 48, 48, 0, 1, 1), (1, 1024, 1, 9, 7, 0, 0, 0),
                                                  (1, 512, 3, 5, 3, 0, 1, 0),
                                                  # >= 512 tiles: the both-output-halves variant of the kernel
                                                  (1, 192, 3, 128, 136, 1, 0, 1), (2, 576, 1, 70, 61, 0, 1, 0),
                                                  # >= 128 blocks of 128 pixels: conv1x1_stream_kernel (ragged last block)
                                                  (1, 576, 1, 256, 128, 0, 1, 1), (2, 1024, 1, 129, 132, 1, 0, 0),
                                                  (1, 64, 1, 200, 164, 0, 0, 1)]:
        total = max(cin, 64) + 64
        buf = torch.randn((b, total, h, w), device=dev, generator=gen)          # input = first cin planes of a larger buffer
        wt = torch.randn((64, cin, k, k), device=dev, generator=gen) / (cin * k * k) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out0 = torch.full((b, 64, h, w), float("nan"), device=dev)
        out1 = torch.full((b, 96, h, w), float("nan"), device=dev) if two else None
        packed = M.pack_conv_ksplit(wt).to(dev)
        st = lib.diinn_conv_ksplit(stream, ptr(buf), total * h * w, cin, k * k, ptr(packed), ptr(bias),
                                  ptr(res) if use_res else None, 64 * h * w, ptr(out0), 64 * h * w,
                                  ptr(out1[:, 32:]) if two else None, 96 * h * w, relu, b, h, w)
        assert st == 0
        torch.cuda.synchronize()
        ref = F.conv2d(buf[:, :cin].double(), wt.double(), bias.double(), padding=k // 2)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out0.double() - ref).abs().max())
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (cin, k, h, w, err)
        if two:
            assert torch.equal(out1[:, 32:96], out0) and torch.isnan(out1[:, :32]).all()
            for _ in range(40):                                  # the two destinations agree on every launch (st_b128 hazard)
                out1[:, 32:].fill_(float("nan"))
                lib.diinn_conv_ksplit(stream, ptr(buf), total * h * w, cin, k * k, ptr(packed), ptr(bias),
                                      ptr(res) if use_res else None, 64 * h * w, ptr(out0), 64 * h * w,
                                      ptr(out1[:, 32:]), 96 * h * w, relu, b, h, w)
                assert torch.equal(out1[:, 32:96], out0)
    assert lib.diinn_conv_ksplit(stream, ptr(buf), 1, 96, 9, ptr(packed), ptr(bias), None, 0, ptr(out0), 1, None, 0, 0, 1, 4, 4) == N.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_conv_t16_kernel_matches_fp64_conv(knobs):
    """diinn_conv_t16 (small maps: strips of 16 pixels x output quarters, 1..3 rows per workgroup, the split-K kernel's weight
    image): ReLU / residual, strided channel-plane views, batches, partly filled strips, single-row maps, every rows-per-
    workgroup form (compute-unit counts forced through DIINN_DEBUG_NCU), against the float64 convolution; repeatable bit for bit;
    and the maps it refuses."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    cases = [(0, 1, 64, 48, 48, 1, 0), (0, 1, 512, 48, 48, 0, 1), (0, 2, 320, 12, 20, 1, 0), (0, 1, 192, 32, 32, 1, 0),
             (0, 1, 128, 40, 40, 0, 0), (0, 1, 448, 16, 16, 1, 0), (0, 4, 256, 24, 24, 1, 1), (0, 1, 64, 1, 4, 0, 0),
             (0, 1, 576, 20, 24, 1, 0), (0, 1, 128, 7, 100, 0, 1),
             # 32 / 128 compute units: 8 / 32 workgroups per output quarter = 3, 2 and 1 rows each on these maps
             (32, 1, 256, 24, 16, 1, 0), (32, 1, 128, 16, 16, 0, 1), (128, 2, 192, 30, 12, 1, 0), (128, 1, 64, 64, 8, 0, 0)]
    for (ncu, b, cin, h, w, relu, use_res) in cases:
        knobs("DIINN_DEBUG_NCU", ncu)
        total = cin + 64
        buf = torch.randn((b, total, h, w), device=dev, generator=gen)          # input = first cin planes of a larger buffer
        wt = torch.randn((64, cin, 3, 3), device=dev, generator=gen) / (cin * 9) ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out = torch.full((b, 96, h, w), float("nan"), device=dev)
        packed = M.pack_conv_ksplit(wt).to(dev)

        def run():
            return lib.diinn_conv_t16(stream, ptr(buf), total * h * w, cin, ptr(packed), ptr(bias), ptr(res) if use_res else None,
                                      64 * h * w, ptr(out[:, 32:]), 96 * h * w, relu, b, h, w)
        assert run() == 0, (ncu, b, cin, h, w)
        torch.cuda.synchronize()
        ref = F.conv2d(buf[:, :cin].double(), wt.double(), bias.double(), padding=1)
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out[:, 32:].double() - ref).abs().max())
        assert err <= 2e-6 * max(1.0, float(ref.abs().max())), (ncu, b, cin, h, w, err)
        assert torch.isnan(out[:, :32]).all()                    # nothing outside the destination planes
        first = out.clone()
        for _ in range(5):
            out.fill_(float("nan"))
            assert run() == 0
            assert torch.equal(out[:, 32:], first[:, 32:])
    knobs("DIINN_DEBUG_NCU", 0)
    # refused: rows not made of whole 16-byte pieces, channels not in runs of 64, more than 3 rows per workgroup, more channels
    # than the kernel's run division is exact for (Cin > 4096: test_conv_t16_weight_run_division_is_exact_where_the_entry_point_accepts)
    small = torch.zeros(1, 128, 64, 64, device=dev)
    o = torch.zeros(1, 64, 64, 64, device=dev)
    for (cin, h, w) in [(64, 8, 6), (96, 8, 8), (64, 64, 64), (4160, 8, 8), (6656, 8, 8)]:
        assert lib.diinn_conv_t16(stream, ptr(small), 128 * h * w, cin, ptr(packed), ptr(bias), None, 0, ptr(o), 64 * h * w, 0, 1, h, w) == N.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_conv1x1_t16_kernel_matches_fp64_conv(knobs):
    """diinn_conv1x1_t16 (the local-fusion layers on small maps; the split-K kernel's 1x1 image): residual, ReLU, two
    destinations, batches, partly filled strips, 1 / 2 / 3 rows per workgroup, against the float64 convolution; repeatable
    bit for bit; and what it refuses."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(6)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    cases = [(0, 1, 576, 48, 48, 0, 1, 1), (0, 1, 576, 32, 32, 0, 1, 1), (0, 2, 576, 24, 40, 0, 1, 1), (0, 1, 64, 17, 52, 1, 0, 0),
             (0, 1, 640, 1, 4, 0, 0, 1), (0, 4, 320, 24, 24, 1, 1, 0), (32, 1, 576, 24, 16, 0, 1, 1), (32, 1, 128, 16, 16, 1, 0, 1),
             (128, 2, 192, 30, 12, 0, 1, 0)]
    for (ncu, b, cin, h, w, relu, use_res, two) in cases:
        knobs("DIINN_DEBUG_NCU", ncu)
        total = cin + 64
        buf = torch.randn((b, total, h, w), device=dev, generator=gen)
        wt = torch.randn((64, cin, 1, 1), device=dev, generator=gen) / cin ** 0.5
        bias = torch.randn(64, device=dev, generator=gen)
        res = torch.randn((b, 64, h, w), device=dev, generator=gen) if use_res else None
        out0 = torch.full((b, 64, h, w), float("nan"), device=dev)
        out1 = torch.full((b, 96, h, w), float("nan"), device=dev) if two else None
        packed = M.pack_conv_ksplit(wt).to(dev)

        def run():
            return lib.diinn_conv1x1_t16(stream, ptr(buf), total * h * w, cin, ptr(packed), ptr(bias), ptr(res) if use_res else None,
                                         64 * h * w, ptr(out0), 64 * h * w, ptr(out1[:, 32:]) if two else None, 96 * h * w, relu, b, h, w)
        assert run() == 0, (ncu, b, cin, h, w)
        torch.cuda.synchronize()
        ref = F.conv2d(buf[:, :cin].double(), wt.double(), bias.double())
        if relu:
            ref = torch.relu(ref)
        if use_res:
            ref = ref + res.double()
        err = float((out0.double() - ref).abs().max())
        assert err <= 2e-6 * max(1.0, float(ref.abs().max())), (ncu, b, cin, h, w, err)
        if two:
            assert torch.equal(out1[:, 32:], out0) and torch.isnan(out1[:, :32]).all()
        first = out0.clone()
        for _ in range(5):
            out0.fill_(float("nan"))
            assert run() == 0
            assert torch.equal(out0, first)
    knobs("DIINN_DEBUG_NCU", 0)
    z = torch.zeros(1, 1088, 8, 8, device=dev)
    o = torch.zeros(1, 64, 64, 64, device=dev)
    for (cin, h, w) in [(1024, 8, 8), (96, 8, 8), (64, 8, 6), (64, 64, 64)]:   # too many channels for one wave's stages, ...
        assert lib.diinn_conv1x1_t16(stream, ptr(z), 1088 * h * w, cin, ptr(packed), ptr(bias), None, 0, ptr(o), 64 * h * w, None, 0, 0, 1, h, w) == N.ERR_UNSUPPORTED


def test_conv_t16_dispatch_rule(knobs):
    """diinn_conv_t16_applies: the maps whose 3x3 layers the trunk gives to the small-map kernel (no device needed: the
    compute-unit count is forced)."""
    import diinn_amd._native as N
    lib = N.load()
    knobs("DIINN_DEBUG_NCU", 256)
    assert lib.diinn_conv_t16_applies(1, 48, 48) == 1           # 144 split-K units on 256 CUs; 3 strips x 48 rows over 64 = 2 or 3 rows
    assert lib.diinn_conv_t16_applies(1, 32, 32) == 1
    assert lib.diinn_conv_t16_applies(1, 40, 40) == 1
    assert lib.diinn_conv_t16_applies(4, 24, 24) == 1
    assert lib.diinn_conv_t16_applies(1, 1, 4) == 1
    assert lib.diinn_conv_t16_applies(1, 64, 64) == 0           # 256 split-K units: every CU has one; 4 rows per workgroup here
    assert lib.diinn_conv_t16_applies(1, 48, 50) == 0           # rows of whole 16-byte pieces only
    assert lib.diinn_conv_t16_applies(1, 128, 128) == 0         # a Winograd map
    assert lib.diinn_conv_t16_applies(0, 48, 48) == 0
    knobs("DIINN_DEBUG_NCU", 64)                                 # a partition of 64 CUs: 16 workgroups per quarter
    assert lib.diinn_conv_t16_applies(1, 48, 48) == 0 and lib.diinn_conv_t16_applies(1, 16, 16) == 1
    knobs("DIINN_DEBUG_NCU", 256)
    knobs("DIINN_ENC_NO_T16", 1)
    assert lib.diinn_conv_t16_applies(1, 48, 48) == 0


def test_conv_t16_partition_covers_every_row_once(knobs):
    """diinn_conv_t16_plan: on every map the kernel takes, the workgroups of a quarter cover every row of every strip exactly
    once with at most 3 rows each and no more workgroups than a quarter of the compute units; and the multiplier form of the
    kernel's divisions (x / d == (x * (2^32 / d + 1)) >> 32) is exact on its whole range."""
    import ctypes as C
    import diinn_amd._native as N
    lib = N.load()
    info = (C.c_int * 4)()
    taken = 0
    for ncu in (256, 304, 128, 64, 20):
        knobs("DIINN_DEBUG_NCU", ncu)
        for b in (1, 2, 3, 5):
            for h in (1, 2, 7, 16, 17, 24, 31, 40, 48, 49, 63, 64, 96, 200):
                for w in (4, 12, 16, 20, 48, 52, 64, 100):
                    assert lib.diinn_conv_t16_plan(b, h, w, info) == 0
                    slots, per_strip, rows, strips = info[0], info[1], info[2], info[3]
                    assert strips == b * ((w + 15) // 16)
                    if lib.diinn_conv_t16_applies(b, h, w):
                        assert slots > 0
                    if slots == 0:
                        continue
                    taken += 1
                    assert slots == strips * per_strip and slots <= max(1, ncu // 4) and 1 <= rows <= 3
                    cover = np.zeros((strips, h), dtype=np.int32)
                    for s in range(slots):
                        strip, j = divmod(s, per_strip)
                        y0 = j * rows
                        n = min(rows, h - y0)
                        assert n >= 1                            # no workgroup without rows
                        cover[strip, y0:y0 + n] += 1
                    assert (cover == 1).all(), (ncu, b, h, w)
    assert taken > 100
    x = np.arange(65536, dtype=np.uint64)
    for d in list(range(2, 300)) + [511, 512, 513, 1000, 4095, 4096, 21845, 32768, 65535]:
        m = np.uint64((1 << 32) // d + 1)
        assert np.array_equal((x * m) >> np.uint64(32), x // np.uint64(d)), d


def test_conv_t16_weight_run_division_is_exact_where_the_entry_point_accepts(knobs):
    """conv_t16_kernel / conv1x1_t16_kernel find the wave of a weight run as r8 / runs = (r8 * inv_runs) >> 16 in 32-bit arithmetic,
    inv_runs = ceil(65536 / runs), runs = Cin / 64, r8 = 2 group + (lane >> 5) < 8 runs (Cin / 16 groups of 16 channels).  Exact
    for every runs <= 103 and first wrong at 104 (Cin = 6656), where a launch would read another wave's weights without a
    word: diinn_conv_t16 stops at Cin = 4096 (include/diinn_hip.h), diinn_conv1x1_t16 at 640, and both refuse more before any
    device call (no device needed here: the compute-unit count is forced and the pointers are never followed)."""
    import ctypes as C
    import diinn_amd._native as N
    lib = N.load()
    max_cin = 4096

    def exact(runs):
        r8 = np.arange(8 * runs, dtype=np.uint32)
        inv = np.uint32((65536 + runs - 1) // runs)
        return np.array_equal((r8 * inv) >> np.uint32(16), r8 // np.uint32(runs))
    for cin in range(64, max_cin + 1, 64):                       # every Cin the entry point accepts
        assert exact(cin // 64), cin
    assert all(exact(runs) for runs in range(max_cin // 64, 104)) and not exact(104)
    knobs("DIINN_DEBUG_NCU", 256)
    fake = C.c_void_p(1 << 20)                                   # non-null, 16-byte aligned; a refused call follows no pointer
    for cin, want in [(max_cin + 64, N.ERR_UNSUPPORTED), (6656, N.ERR_UNSUPPORTED), (1 << 20, N.ERR_UNSUPPORTED), (96, N.ERR_UNSUPPORTED)]:
        assert lib.diinn_conv_t16(None, fake, cin * 64, cin, fake, fake, None, 0, fake, 64 * 64, 0, 1, 8, 8) == want, cin
    for cin in (704, max_cin + 64):
        assert lib.diinn_conv1x1_t16(None, fake, cin * 64, cin, fake, fake, None, 0, fake, 64 * 64, None, 0, 0, 1, 8, 8) == N.ERR_UNSUPPORTED, cin


@pytest.mark.gpu
def test_rdn_trunk_small_map_kernel_against_the_split_k_kernel(knobs):
    """The trunk on maps the small-map kernel takes (48 x 48: the reference's timing protocol, runtime_test.py:13) equals the
    trunk with that kernel switched off (DIINN_ENC_NO_T16: split-K everywhere) up to the order of the fp32 sums, and MIOpen."""
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    enc = M.make_rdn()
    shapes = {k: list(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(shapes, 31, "enc.").items()})
    enc = enc.to(dev).eval()
    for (b, h, w) in [(1, 48, 48), (1, 32, 32), (2, 24, 40), (1, 17, 52)]:
        assert N.load().diinn_conv_t16_applies(b, h, w) == 1
        x = torch.from_numpy(synth.uniform(9, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
        with torch.no_grad():
            got = enc(x)
            knobs("DIINN_ENC_NO_T16", 1)
            ks = enc(x)
            knobs("DIINN_ENC_NO_T16", 0)
            enc.hip_trunk_max_pixels = None
            ref = enc(x)
            enc.hip_trunk_max_pixels = M.RDN.hip_trunk_max_pixels
        scale = max(1.0, float(ref.abs().max()))
        assert not torch.equal(got, ks)                          # (another kernel did run)
        if (b, h, w) == (1, 48, 48):
            with torch.no_grad():
                for _ in range(90):                              # back-to-back forwards repeat bit for bit
                    assert torch.equal(enc(x), got)
            # shallow features that are not 16-byte aligned (the strip kernel stages 16-byte pieces): the split-K kernel, as before
            import ctypes as C
            lib = N.load()
            ptr = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
            with torch.no_grad():
                sfe1 = enc._sfe1_hip(x)
            shifted = torch.empty(sfe1.numel() + 1, device=dev)[1:].view_as(sfe1).copy_(sfe1)
            assert shifted.data_ptr() % 16 == 4
            packed, biases = enc._hip_packed(dev)
            planes = torch.empty(lib.diinn_rdn_planes_floats(N.RDN_ALGO_DIRECT, b, h, w), device=dev)
            out = torch.empty_like(sfe1)
            assert lib.diinn_rdn_forward_ex(C.c_void_p(torch.cuda.current_stream().cuda_stream), N.RDN_ALGO_DIRECT, ptr(shifted), ptr(packed),
                                            None, None, None, ptr(biases), ptr(planes), None, ptr(out), b, h, w) == 0
            torch.cuda.synchronize()
            assert torch.equal(out, ks)
        assert float((got - ks).abs().max()) <= 5e-6 * scale, (b, h, w)
        assert float((got - ref).abs().max()) <= 2e-5 * scale, (b, h, w)


@pytest.mark.gpu
def test_rdn_hip_trunk_matches_miopen():
    """RDN.forward with the HIP trunk (small maps, no grad) against the same module on PyTorch-ROCm/MIOpen."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    enc = M.make_rdn()
    shapes = {k: list(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(shapes, 123, "enc.").items()})
    enc = enc.to(dev).eval()
    # up to 8192 pixels the split-K kernel ((1,70,112)); from there on Winograd 3x3 layers, one
    # output half per workgroup below 448 blocks ((1,160,112), (2,128,130)), both from there on ((1,250,260))
    # (2,200,180): 600 blocks over two images on 256 persistent workgroups
    for (b, h, w) in [(1, 48, 48), (2, 20, 33), (1, 70, 112), (1, 160, 112), (1, 200, 180), (2, 128, 130), (1, 250, 260),
                      (2, 200, 180)]:
        x = torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
        with torch.no_grad():
            got = enc(x)
            enc.hip_trunk_max_pixels = None
            ref = enc(x)
            enc.hip_trunk_max_pixels = M.RDN.hip_trunk_max_pixels
        err = float((got - ref).abs().max())
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (b, h, w, err)
    y = enc(x)                                               # grad enabled: the autograd (PyTorch) path
    assert y.requires_grad


@pytest.mark.gpu
def test_rdn_hip_trunk_odd_shapes():
    """Degenerate and ragged maps (single pixel, single row / column, sizes that are not multiples of the 8x4 tile,
    batch > 1) through the whole HIP trunk against MIOpen."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    enc = M.make_rdn().to(dev).eval()
    for (b, h, w) in [(1, 1, 1), (1, 1, 13), (1, 11, 1), (2, 3, 2), (1, 37, 5), (3, 9, 10), (1, 4, 8), (1, 5, 9)]:
        x = torch.rand(b, 3, h, w, device=dev)
        with torch.no_grad():
            got = enc(x)
            enc.hip_trunk_max_pixels = None
            ref = enc(x)
            enc.hip_trunk_max_pixels = M.RDN.hip_trunk_max_pixels
        assert got.shape == ref.shape == (b, 64, h, w)
        err = float((got - ref).abs().max())
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (b, h, w, err)


@pytest.mark.gpu
def test_rdn_trunk_on_wino4_layers(knobs):
    """The whole encoder with its 130 3x3 layers on diinn_conv_wino4 (forced on at small / ragged maps through the knobs;
    the last three take it by the dispatch rule) against MIOpen: features within 2e-5 of max|feat|
    (measured 1.5e-6; F(2x2): 4e-7), and the image decoded from them within 1e-6 of the one from the F(2x2) features
    (the north_star bound is 1e-4).  RDN.hip_winograd4 = False switches it off."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    net = M.DIINN(mode=3, init_q=False).to(dev).eval()
    enc = net.encoder
    worst = 0.0
    with torch.no_grad():
        for (b, h, w, force) in [(1, 48, 48, 1), (2, 20, 33, 1), (1, 37, 5, 1), (3, 9, 10, 1), (1, 70, 112, 1), (1, 130, 129, 1),
                                 (1, 250, 256, 0), (1, 200, 180, 0), (4, 96, 100, 0)]:
            if force:
                knobs("DIINN_ENC_WINO_MIN", 0)
                knobs("DIINN_ENC_WINO4_MIN", 0)
            else:
                knobs("DIINN_ENC_WINO_MIN", 8192)
                knobs("DIINN_ENC_WINO4_MIN", -1)
            x = torch.rand(b, 3, h, w, device=dev)
            enc.hip_winograd4 = True
            f4 = enc(x)
            enc.hip_winograd4 = False
            f2 = enc(x)
            enc.hip_trunk_max_pixels = None
            ref = enc(x)
            enc.hip_trunk_max_pixels = M.RDN.hip_trunk_max_pixels
            enc.hip_winograd4 = True
            scale = max(1.0, float(ref.abs().max()))
            err = float((f4 - ref).abs().max())
            assert err <= 2e-5 * scale, (b, h, w, err)
            worst = max(worst, err / scale)
            assert not torch.equal(f4, f2), (b, h, w)             # the other kernel did run
            if h * w <= 130 * 129:
                size = (2 * h + 3, 3 * w - 1)
                assert float((net.decoder(f4, size, 30000) - net.decoder(f2, size, 30000)).abs().max()) <= 1e-6, (b, h, w)
    print(f"trunk on F(4x4,3x3) layers: worst error {worst:.2e} of max|feat|")


@pytest.mark.gpu
def test_graph_capture_with_wino4_layers():
    """DIINN(graphs=True) on a map whose 3x3 layers take diinn_conv_wino4 (the F(4x4) weight image is packed in the warm-up,
    kept alive by the graph entry): replays equal the eager forward bit for bit, also for new input contents."""
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = M.DIINN(mode=3, init_q=False).to(dev).eval()
    assert N.load().diinn_rdn_wino4_applies(1, 200, 180) == 1
    x, x2 = torch.rand(1, 3, 200, 180, device=dev), torch.rand(1, 3, 200, 180, device=dev)
    with torch.no_grad():
        ref, ref2 = net(x, (400, 360)), net(x2, (400, 360))
        net.graphs = True
        assert torch.equal(net(x, (400, 360)), ref) and torch.equal(net(x, (400, 360)), ref)
        assert torch.equal(net(x2, (400, 360)), ref2)
        net.graphs = False


@pytest.mark.gpu
def test_rdn_hip_trunk_matches_the_reference_on_big_maps():
    """RDN.forward on maps that take the Winograd 3x3 kernels (one half / both halves per workgroup) and the streaming
    1x1 kernel, against the REAL reference's encoder run on the CPU: 16,384 sampled outputs and per-channel sums from
    tests/golden/rdn_big_golden.npz (tests/golden/make_golden_rdn_big.py imports /root/reference's make_rdn)."""
    import json
    import os
    import diinn_amd.modules as M
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rdn_big_golden.npz"))
    dev = torch.device("cuda:0")
    enc = M.make_rdn()
    shapes = json.loads(str(gold["rdn/shapes_json"]))
    assert shapes == {k: list(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(shapes, 123, "enc.").items()})
    enc = enc.to(dev).eval()
    for (b, h, w) in [(1, 96, 100), (1, 240, 256), (2, 50, 90)]:
        key = f"{b}x{h}x{w}"
        x = torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
        with torch.no_grad():
            y = enc(x).cpu().numpy()
        idx = np.random.default_rng(1000 * h + w).choice(y.size, size=min(16384, y.size), replace=False)
        scale = max(1.0, float(gold[f"rdn/{key}/absmax"]))
        err = float(np.abs(y.reshape(-1)[idx] - gold[f"rdn/{key}/values"]).max())
        assert err <= 2e-5 * scale, (key, err)
        sums = y.astype(np.float64).sum(axis=(0, 2, 3))
        assert float(np.abs(sums - gold[f"rdn/{key}/channel_sums"]).max()) <= 1e-6 * b * h * w * scale, key


def _gold_r5():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diinn_golden_r5.npz"))


@pytest.mark.gpu
def test_rdn_trunk_regression_bound_on_big_maps():
    """The regression-level bound beside the 2e-5 contract of test_rdn_hip_trunk_matches_the_reference_on_big_maps (VERDICT r04
    item 4c): on the 240 x 256 fixture -- F(4x4,3x3) layers, the default arithmetic of big maps -- the sampled features are
    within 6e-6 of max|ref| of the real reference's (3x the 2e-6 measured when the kernel shipped); on the two maps that run
    F(2x2,3x3) within 2e-6 (measured 5e-7)."""
    import json
    import os
    import diinn_amd._native as N
    import diinn_amd.modules as M
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rdn_big_golden.npz"))
    dev = torch.device("cuda:0")
    enc = M.make_rdn()
    shapes = json.loads(str(gold["rdn/shapes_json"]))
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(shapes, 123, "enc.").items()})
    enc = enc.to(dev).eval()
    lib = N.load()
    for (b, h, w) in [(1, 96, 100), (1, 240, 256), (2, 50, 90)]:
        key = f"{b}x{h}x{w}"
        x = torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
        with torch.no_grad():
            y = enc(x).cpu().numpy()
        idx = np.random.default_rng(1000 * h + w).choice(y.size, size=min(16384, y.size), replace=False)
        scale = max(1.0, float(gold[f"rdn/{key}/absmax"]))
        err = float(np.abs(y.reshape(-1)[idx] - gold[f"rdn/{key}/values"]).max())
        f4 = bool(lib.diinn_rdn_wino4_applies(b, h, w))
        print(f"{key}: F({'4x4' if f4 else '2x2'},3x3) layers, |hip - ref| {err:.2e} of max|ref| {scale:.2f}")
        assert err <= (6e-6 if f4 else 2e-6) * scale, (key, err)


@pytest.mark.gpu
def test_diinn_forward_matches_the_reference_on_a_map_with_wino4_layers():
    """ONE assertion for the whole model on a map whose encoder takes the default arithmetic of big maps:
    DIINN.forward (RDN encoder with F(4x4,3x3) layers, the last round split over the input channels; then the implicit decoder) on
    a 200 x 180 image -> 431 x 377 against the REAL reference's DIINN (src/models/components/diinn.py:8-19) run on the CPU: 16,384
    sampled outputs from tests/golden/diinn_golden_r5.npz (make_golden_r5.py), per-channel sums; north_star bound
    1e-4 x max(1, |ref|), and -- informational -- the distance to the same model run in float64 beside the reference's own."""
    import json
    import diinn_amd._native as N
    import diinn_amd.modules as M
    gold = _gold_r5()
    dev = torch.device("cuda:0")
    net = M.DIINN(mode=3, init_q=False)
    full = json.loads(str(gold["diinn/shapes_json"]))
    assert full == {k: list(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(full, 123, "diinn.").items()})
    net = net.to(dev).eval()
    b, h, w, hu, wu = 1, 200, 180, 431, 377
    assert N.load().diinn_rdn_wino4_applies(b, h, w) == 1
    key = f"diinn/{h}x{w}_{hu}x{wu}"
    x = torch.from_numpy(synth.uniform(11, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
    with torch.no_grad():
        y = net(x, [hu, wu], 30000).cpu().numpy()
    assert y.shape == (b, 3, hu, wu)
    idx = np.random.default_rng(1000 * hu + wu).choice(y.size, size=16384, replace=False)
    got = y.reshape(-1)[idx]
    ref, ref64 = gold[f"{key}/values"], gold[f"{key}/values64"]
    scale = max(1.0, float(gold[f"{key}/absmax"]))
    err = float(np.abs(got - ref).max())
    err64, ref_err64 = float(np.abs(got - ref64).max()), float(np.abs(ref - ref64).max())
    print(f"DIINN 200x180 -> 431x377: |hip - ref32| {err:.2e}; against float64: hip {err64:.2e}, the reference itself {ref_err64:.2e}")
    assert err <= 1e-4 * scale, err
    assert err <= 5e-7, err                                      # regression level (measured 4.8e-8 when the fixture was made)
    assert err64 <= 1e-7, err64                                  # ... and against float64 8e-9: closer than the reference itself (4.7e-8)
    sums = y.astype(np.float64).sum(axis=(0, 2, 3))
    assert float(np.abs(sums - gold[f"{key}/channel_sums"]).max()) <= 1e-6 * hu * wu * scale


@pytest.mark.gpu
def test_rdn_trunk_off_default_init_gains(knobs):
    """How the F(4x4,3x3) error grows off the default initialisation: the reference's encoder with every
    weight and bias scaled by 1.5 and by 2.0 (max|feat| 1.5 -> 4.4 -> 75; a trained RDN has per-layer gains of its own and
    no checkpoint is shipped) on a 192 x 200 map, fixtures from the real reference in fp32 and float64.  Contract: 2e-5 x
    max|ref| against the fp32 reference.  Measured against float64, relative to max|ref| (gain 1 -> 1.5 -> 2.0): F(4x4) layers
    1.5e-6 -> 3.4e-6 -> 4.4e-6, F(2x2) layers 4e-7 -> 4.9e-7 -> 1.3e-6, the fp32 reference itself 3e-7 -> 4.6e-7 -> 1.2e-6: the
    F(4x4) error grows no faster than the reference's own rounding noise and stays 4-7x above it, a factor 4 inside the
    contract at gain 2.  Regression bounds: 8e-6 (F(4x4)) and 2.5e-6 (F(2x2)) of max|ref| against float64."""
    import json
    import diinn_amd.modules as M
    gold = _gold_r5()
    dev = torch.device("cuda:0")
    enc = M.make_rdn()
    shapes = json.loads(str(gold["rdn/shapes_json"]))
    b, h, w = 1, 192, 200
    x = torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
    for gain in (1.5, 2.0):
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(shapes, 123, "enc.", gain=gain).items()})
        enc = enc.to(dev).eval()
        key = f"rdn_gain/{gain}/{b}x{h}x{w}"
        ref, ref64 = gold[f"{key}/values"], gold[f"{key}/values64"]
        scale = max(1.0, float(gold[f"{key}/absmax"]))
        ref_err64 = float(np.abs(ref - ref64).max())
        for f4 in (True, False):
            enc.hip_winograd4 = f4
            with torch.no_grad():
                y = enc(x).cpu().numpy()
            idx = np.random.default_rng(1000 * h + w).choice(y.size, size=16384, replace=False)
            got = y.reshape(-1)[idx]
            err, err64 = float(np.abs(got - ref).max()), float(np.abs(got - ref64).max())
            print(f"gain {gain}, F({'4x4' if f4 else '2x2'},3x3): |hip - ref32| {err / scale:.2e} of max|ref| {scale:.1f}; against float64 "
                  f"{err64 / scale:.2e} (the reference itself {ref_err64 / scale:.2e})")
            assert err <= 2e-5 * scale, (gain, f4, err)
            assert err64 <= (8e-6 if f4 else 2.5e-6) * scale, (gain, f4, err64, ref_err64)
    enc.hip_winograd4 = True


def test_layer_gains_are_deterministic():
    """synth.layer_gain: the per-layer gains of the round-6 fixtures (2^u, u in (-0.6, 1.0)) depend on (seed, layer name) only."""
    g = [synth.layer_gain(77, f"enc.RDBs.{d}.convs.{c}.conv.0") for d in range(16) for c in range(8)]
    assert g == [synth.layer_gain(77, f"enc.RDBs.{d}.convs.{c}.conv.0") for d in range(16) for c in range(8)]
    assert 0.659 < min(g) and max(g) < 2.0001 and len({round(x, 6) for x in g}) > 100
    assert synth.layer_gain(77, "enc.SFENet2") != synth.layer_gain(78, "enc.SFENet2")
    shapes = {"a.weight": [64, 64, 3, 3], "a.bias": [64], "b.weight": [64, 128, 1, 1], "b.bias": [64]}
    plain = synth.state_dict_for(shapes, 5, "m.")
    gained = synth.state_dict_for(shapes, 5, "m.", layer_gain_seed=9)
    for layer in ("a", "b"):
        ga = synth.layer_gain(9, "m." + layer)
        for t in ("weight", "bias"):                              # weight and bias of a layer share its gain
            assert np.allclose(gained[f"{layer}.{t}"], plain[f"{layer}.{t}"] * np.float32(ga), rtol=2e-7, atol=0)


@pytest.mark.gpu
def test_rdn_trunk_with_per_layer_gains():
    """VERDICT r05, weak item 3 ("encoder parity off default init is one map, two gains"): the reference's encoder with a gain of
    its own in EVERY layer (2^u, u ~ U(-0.6, 1.0): what a trained network looks like to a Winograd transform's rounding, unlike a
    uniformly scaled default init) on one map per kernel family of the trunk -- 256 x 256 (F(4x4), an exact round), 320 x 180
    (F(4x4) with the last round split), 100 x 120 (F(2x2)), 2 x 48 x 48 (split-K) -- fixtures from the real reference in fp32
    and float64 (tests/golden/make_golden_r6.py).  Contract: 2e-5 x max|ref| against the fp32 reference; regression bounds
    against float64 per family (printed: the reference's own fp32 noise beside ours)."""
    import json
    import os
    import diinn_amd._native as N
    import diinn_amd.modules as M
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diinn_golden_r6.npz"))
    dev = torch.device("cuda:0")
    lib = N.load()
    enc = M.make_rdn()
    shapes = json.loads(str(gold["rdn/shapes_json"]))
    for (gseed, b, h, w, bound64) in [(77, 1, 256, 256, 8e-6), (77, 1, 320, 180, 8e-6), (78, 1, 100, 120, 2.5e-6), (78, 2, 48, 48, 2.5e-6)]:
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(shapes, 123, "enc.", layer_gain_seed=gseed).items()})
        enc = enc.to(dev).eval()
        x = torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
        key = f"rdn_layer_gain/{gseed}/{b}x{h}x{w}"
        ref, ref64 = gold[f"{key}/values"], gold[f"{key}/values64"]
        scale = max(1.0, float(gold[f"{key}/absmax"]))
        with torch.no_grad():
            y = enc(x).cpu().numpy()
        idx = np.random.default_rng(1000 * h + w).choice(y.size, size=min(16384, y.size), replace=False)
        got = y.reshape(-1)[idx]
        err, err64, ref_err64 = float(np.abs(got - ref).max()), float(np.abs(got - ref64).max()), float(np.abs(ref - ref64).max())
        fam = "F(4x4)" if lib.diinn_rdn_wino4_applies(b, h, w) else "F(2x2)" if b * h * w >= 8192 else "split-K"
        print(f"{key} [{fam}]: |hip - ref32| {err / scale:.2e} of max|ref| {scale:.2f}; against float64 {err64 / scale:.2e} "
              f"(the reference itself {ref_err64 / scale:.2e})")
        assert np.isfinite(got).all()
        assert err <= 2e-5 * scale, (key, err)
        assert err64 <= bound64 * scale, (key, err64, ref_err64)


def _check_against_r7(y, gold, key, seed, bound32, bound64, label):
    """One output against a round-7 fixture: sampled values (fp32 reference: `bound32`; the same model in float64: `bound64`,
    None = printed only; both relative to max(1, max|ref|)), per-channel sums over the WHOLE tensor, every value finite.
    Returns the two distances, relative to that scale."""
    assert np.isfinite(y).all(), (key, label)
    idx = np.random.default_rng(seed).choice(y.size, size=min(16384, y.size), replace=False)
    got = y.reshape(-1)[idx]
    ref, ref64 = gold[f"{key}/values"], gold[f"{key}/values64"]
    assert got.shape == ref.shape
    scale = max(1.0, float(gold[f"{key}/absmax"]))
    err, err64, ref_err64 = float(np.abs(got - ref).max()), float(np.abs(got - ref64).max()), float(np.abs(ref - ref64).max())
    sums = y.astype(np.float64).sum(axis=(0, 2, 3))
    sum_err = float(np.abs(sums - gold[f"{key}/channel_sums"]).max())
    print(f"{key} [{label}]: |hip - ref32| {err / scale:.2e} of max(1, max|ref| {float(gold[f'{key}/absmax']):.3f}); against float64 "
          f"{err64 / scale:.2e} (the reference itself {ref_err64 / scale:.2e}); channel sums off by {sum_err:.2e}")
    assert err <= bound32 * scale, (key, label, err)
    if bound64 is not None:
        assert err64 <= bound64 * scale, (key, label, err64, ref_err64)
    assert sum_err <= 1e-6 * (y.size // y.shape[1]) * scale, (key, label, sum_err)
    return err / scale, err64 / scale


@pytest.mark.gpu
def test_rdn_trunk_on_small_map_kernels_matches_the_reference(knobs):
    """conv_t16_kernel / conv1x1_t16_kernel -- the default kernels of every B = 1 map up to about 48 x 48,
    the reference's own timing protocol among them -- against the REAL reference's encoder (per-layer gains as in round 6; fp32 and
    float64 fixtures: tests/golden/make_golden_r7.py) on 1 x 48 x 48 (3 strips x 16 workgroups of 3 rows), 1 x 60 x 40 (3 rows, the
    last strip half filled), 1 x 12 x 12 (1 row per workgroup, one partly filled strip; compared whole), 1 x 36 x 52 (the last strip one
    16-byte piece) and 4 x 24 x 24 (a batch).  Each map runs twice: on the small-map kernels, and with DIINN_ENC_NO_T16 = 1 on the
    split-K kernel (its first B = 1 reference fixtures); the two results differ in bits (the small-map kernels did run) and BOTH meet:
    the encoder contract 2e-5 x max(1, max|ref|) against the fp32 reference; the direct-sum family's 2.5e-6 against float64
    (test_rdn_trunk_with_per_layer_gains); the channel sums of the whole tensor within 1e-6 x B H W x scale; every value finite.
    Measured (MI355X), relative to max(1, max|ref|), |hip - ref32| / |hip - ref64| beside the reference's own |ref32 - ref64|:
        map          t16: ref32 / float64     split-K: ref32 / float64    the reference itself (sampled)
        1x48x48      4.5e-7 / 3.0e-7          4.8e-7 / 2.7e-7             3.6e-7
        1x60x40      4.6e-7 / 2.7e-7          4.0e-7 / 2.4e-7             3.7e-7
        1x12x12      3.1e-7 / 2.4e-7          2.8e-7 / 2.0e-7             2.7e-7
        1x36x52      3.4e-7 / 2.6e-7          3.5e-7 / 2.3e-7             2.5e-7
        4x24x24      3.9e-7 / 3.4e-7          3.6e-7 / 2.5e-7             2.4e-7
    -- both kernels sit at the reference's own fp32 noise, 7x inside the 2.5e-6 bound and 40x inside the contract; channel sums off
    by 2.4e-6 .. 3.5e-5 (bound 1.6e-4 .. 3.4e-3)."""
    import json
    import os
    import diinn_amd._native as N
    import diinn_amd.modules as M
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diinn_golden_r7.npz"))
    dev = torch.device("cuda:0")
    lib = N.load()
    enc = M.make_rdn()
    shapes = json.loads(str(gold["rdn/shapes_json"]))
    assert shapes == {k: list(v.shape) for k, v in enc.state_dict().items()}
    for (gseed, b, h, w) in [(79, 1, 48, 48), (79, 1, 60, 40), (80, 1, 12, 12), (80, 1, 36, 52), (79, 4, 24, 24)]:
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(shapes, 123, "enc.", layer_gain_seed=gseed).items()})
        enc = enc.to(dev).eval()
        x = torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
        key = f"rdn_layer_gain/{gseed}/{b}x{h}x{w}"
        assert lib.diinn_conv_t16_applies(b, h, w) == 1, key
        with torch.no_grad():
            got = enc(x)
            knobs("DIINN_ENC_NO_T16", 1)
            assert lib.diinn_conv_t16_applies(b, h, w) == 0
            ks = enc(x)
            knobs("DIINN_ENC_NO_T16", 0)
        assert got.shape == ks.shape == (b, 64, h, w)
        assert not torch.equal(got, ks), key                     # (the small-map kernels did run)
        for y, label in ((got, "t16"), (ks, "split-K")):
            _check_against_r7(y.cpu().numpy(), gold, key, 1000 * h + w, 2e-5, 2.5e-6, label)


@pytest.mark.gpu
def test_diinn_forward_matches_the_reference_at_the_protocol_geometry():
    """The whole model where the reference times it (runtime_test.py: 1 x 3 x 48 x 48 -> 96 x 96; the encoder on the small-map
    kernels, the decoder on its 16-pixel latency kernel) and on a benchmarks.py x8 map at a non-integer scale (60 x 40 -> 189 x 126),
    against the REAL reference's DIINN(mode=3, init_q=False) run on the CPU (tests/golden/make_golden_r7.py): 16,384 sampled outputs,
    per-channel sums of the whole image; the bounds of test_diinn_forward_matches_the_reference_on_a_map_with_wino4_layers: north_star
    1e-4 x max(1, |ref|), regression level 5e-7 absolute against the fp32 reference.  Printed: the distance to the same model in
    float64 beside the reference's own (3.1e-8 and 5.7e-8).  Measured (MI355X): 48 x 48 -> 96 x 96 |hip - ref32| 3.0e-8, against
    float64 8.1e-9 (the reference itself 3.0e-8 on the samples); 60 x 40 -> 189 x 126 4.5e-8, against float64 8.2e-9 (the reference
    4.4e-8); channel sums off by 1.1e-5 and 2.7e-5 (bound 9.2e-3 and 2.4e-2)."""
    import json
    import os
    import diinn_amd._native as N
    import diinn_amd.modules as M
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diinn_golden_r7_e2e.npz"))
    dev = torch.device("cuda:0")
    net = M.DIINN(mode=3, init_q=False)
    full = json.loads(str(gold["diinn/shapes_json"]))
    assert full == {k: list(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(full, 123, "diinn.").items()})
    net = net.to(dev).eval()
    for (b, h, w, hu, wu) in [(1, 48, 48, 96, 96), (1, 60, 40, 189, 126)]:
        assert N.load().diinn_conv_t16_applies(b, h, w) == 1
        key = f"diinn/{h}x{w}_{hu}x{wu}"
        x = torch.from_numpy(synth.uniform(11, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5)).to(dev)
        with torch.no_grad():
            y = net(x, [hu, wu], 30000).cpu().numpy()
        assert y.shape == (b, 3, hu, wu)
        err, _ = _check_against_r7(y, gold, key, 1000 * hu + wu, 1e-4, None, "whole model")
        assert err <= 5e-7, (key, err)                           # regression level, absolute: max(1, max|ref| 0.055) = 1


# ---------------------------------------------------------------------------------------------------------------------
# split-bf16 3x3 layers (csrc/diinn_conv_x3.hip; optional, RDN.hip_split_bf16)


@pytest.mark.gpu
def test_conv3x3_split_bf16_matches_float64(knobs):
    """diinn_conv3x3_x3 against a float64 convolution: both kernel forms (1 / 2 pixel rows per wave), ragged map sizes
    (zero padding at every border, partial tiles), batches, ReLU, the residual input, a strided destination.  Bound:
    2e-5 of max|out| (measured 2e-6 .. 5e-6: hi + lo bf16 operands carry 16 bits)."""
    import ctypes as C
    import diinn_amd._native as N
    import diinn_amd.modules as M
    lib = N.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rows in (1, 2, 3):                                        # one row / two rows (ring) / two rows + a group's weights in registers
        knobs("DIINN_ENC_X3_ROWS", rows)
        for (b, cin, h, w, relu, use_res) in [(1, 64, 48, 48, 1, 0), (2, 320, 13, 21, 1, 0), (1, 512, 5, 3, 0, 1),
                                              (1, 128, 33, 70, 1, 0), (3, 16, 9, 65, 0, 1), (1, 576, 1, 1, 1, 0)]:
            x = torch.randn(b, cin, h, w, device=dev)
            wt = (torch.rand(64, cin, 3, 3, device=dev) * 2 - 1) / (cin * 9) ** 0.5 * 1.7
            bias = torch.randn(64, device=dev) * 0.1
            res = torch.randn(b, 64, h, w, device=dev) if use_res else None
            ref = torch.nn.functional.conv2d(x.double(), wt.double(), bias.double(), padding=1)
            if relu:
                ref = ref.relu()
            if use_res:
                ref = ref + res.double()
            wx = M.pack_conv_x3(wt).to(dev)
            assert wx.numel() == 9 * 64 * cin
            big = torch.full((b, 96, h, w), float("nan"), device=dev)          # destination: channels 16..79 of a wider buffer
            out = big[:, 16:80]
            N.check(lib.diinn_conv3x3_x3(st, C.c_void_p(x.data_ptr()), cin * h * w, cin, C.c_void_p(wx.data_ptr()),
                                         C.c_void_p(bias.data_ptr()), C.c_void_p(res.data_ptr()) if use_res else None,
                                         64 * h * w, C.c_void_p(out.data_ptr()), 96 * h * w, relu, b, h, w), "diinn_conv3x3_x3")
            torch.cuda.synchronize()
            scale = float(ref.abs().max())
            err = float((out.double() - ref).abs().max())
            assert err <= 2e-5 * scale, (rows, b, cin, h, w, err / scale)
            assert bool(torch.isnan(big[:, :16]).all()) and bool(torch.isnan(big[:, 80:]).all())   # nothing outside the 64 planes
    # shapes it does not cover are refused
    assert lib.diinn_conv3x3_x3(st, C.c_void_p(x.data_ptr()), 0, 24, C.c_void_p(wx.data_ptr()), C.c_void_p(bias.data_ptr()),
                                None, 0, C.c_void_p(out.data_ptr()), 0, 0, 1, 8, 8) == N.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_trunk_with_split_bf16_layers_tracks_the_fp32_trunk(knobs):
    """RDN.hip_split_bf16: the whole encoder with its 130 3x3 layers on diinn_conv3x3_x3 (forced on at a small map through
    DIINN_ENC_X3_MIN) against the fp32 trunk: features within 3e-5 of max|feat| (measured 3e-6), and the image decoded
    from them within 1e-6 (measured 2e-8; the north_star bound is 1e-4) -- the per-layer 4e-6 does not pile up."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    net = M.DIINN(mode=3, init_q=False).to(dev).eval()
    enc = net.encoder
    knobs("DIINN_ENC_X3_MIN", 0)
    with torch.no_grad():
        for (b, h, w, form) in [(1, 96, 100, 0), (2, 40, 72, 0), (1, 45, 67, 4), (1, 64, 40, 2), (1, 33, 35, 1)]:
            knobs("DIINN_ENC_X3_ROWS", form)                      # 0: the launcher's choice; every kernel form inside the trunk
            x = torch.rand(b, 3, h, w, device=dev)
            enc.hip_split_bf16 = False
            f32 = enc(x)
            enc.hip_split_bf16 = True
            f3 = enc(x)
            assert float((f3 - f32).abs().max()) <= 3e-5 * float(f32.abs().max()), (b, h, w)
            assert not torch.equal(f3, f32)                          # the other kernel did run
            size = (2 * h + 3, 3 * w - 1)
            img32, img3 = net.decoder(f32, size, 30000), net.decoder(f3, size, 30000)
            assert float((img3 - img32).abs().max()) <= 1e-6, (b, h, w)
    enc.hip_split_bf16 = False
