// diinn_initq.hip -- decoder init_q=True: the per-pixel sine embedding and the two per-pixel GEMMs it forces (every mode's planes)
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, image and plane layout in diinn_layout.h)
//
// Reference path replaced: ImplicitDecoder.step with init_q (diinn.py:48-51,113-115):
//   E  = sin(first_layer . (rel_h, rel_w, ratio) + bF)      576 values per HR pixel
//   x' = E * X[cell]                                         X = unfold3x3(feat) of the pixel's LR cell (zero padded)
// and every layer reads x' where it read X, Q.0 reads E.  x' depends on the HR pixel, so the hoisted conv per LR cell
// (precompute_P_kernel) is gone: per pixel,
//   PIX[0..1023]    = Wx . x' + bK                           (1024 x 576; what P[cell] holds when init_q is off)
//   PIX[1024..1279] = (Q0 . E + bQ0) / (2 pi)                (256 x 576; layer 0's sine argument, in revolutions)
// decode_kernel<SIN | DECODE_INITQ> (diinn_decode.hip) runs the layers and the head from these planes (mode 3; modes 1/2 after
// pixel_chain_kernel, mode 4 in its tap form: see there).  Mode 1 needs channels 0..255 and 1024..1279 only: INITQ_ROWS512.
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// initq_planes_kernel: a GEMM [1280 x 576] . [576 x pixels] on v_mfma_f32_32x32x2_f32, designed from precompute_P_kernel.
// Workgroup = 4 waves = an 8 x 8 tile of HR pixels = two N-tiles of 8 x 4 (decode_kernel's wave tile).  The B operand of the
// whole tile lives in ONE LDS buffer [k-step 288][N-tile 2][lane 64] (144 KiB of the CU's 160), filled twice:
//   pass 1  E       -> every wave runs one M-tile pair of Q0 (the init_q image's Q0W pieces): channels 1024 + 64 wave ..
//   pass 2  E * X in place (each thread owns the slots it wrote; X by clamped loads and a select, zero outside the map)
//           -> every wave runs four M-tile pairs of WP (the body image's section 1): channels 256 wave .. 256 wave + 255.
// A wave keeps both N-tiles' accumulators of its pair (4 x 16 registers), so a 1 KiB weight piece feeds 8 MFMAs (2 B / clock
// / wave from the L2; the four waves stream different pieces) and a k-step's two B values are two ds_read_b32 at immediate
// offsets.  Results leave through a per-wave LDS transpose, 16 channels of 32 pixels at a time, so that four lanes write 64
// contiguous bytes of a pixel's record (the LDS left beside the B buffer holds no wider transpose).
// A pixel's arithmetic depends on nothing but the pixel: bands and chunks of rows are bit-identical to the whole image.
// No atomics, no scratch, one workgroup per CU.
// ---------------------------------------------------------------------------------
struct InitqParams {
    const float* feat;   // [B,64,H,W]
    const float* Wt;     // body image (sections WP, BK)
    const float* iq;     // init_q image (diinn_pack_initq)
    float* pix;          // [B][y1 - y0][Wu][PIX_CH]
    int B, H, W, Hu, Wu, y0, y1;
    float ratio;         // fp32(H*W / (Hu*Wu))   (diinn.py:166)
    Axis ah, aw;
    int stream_stores;   // the planes are larger than the last-level cache: write them with streaming (nt) stores
};

constexpr int IQ_TW = 8, IQ_TH = 8;                       // HR pixels per workgroup: two N-tiles of 8 x 4
constexpr int IQ_BUF = WP_KSTEPS * 2 * 64;                // 36,864 floats = 147,456 B
constexpr int IQ_TR_PITCH = 20;                           // floats per pixel in the store transpose (16 + 4)
constexpr int IQ_ITERS = IQ_BUF / 256;                    // 144 slots per thread and pass

// INITQ_RAD (the training forward, diinn_decode_initq_train_fwd): `iq` is the init_q TRAINING image, whose F / Q0W / BQ0 part is
// in radians (a pure permutation of the reference tensors: diinn_layout.h), so E = sin(a) takes a in radians and channels
// 1024..1279 leave in radians, as decode_kernel<SIN | DECODE_INITQ, true, SAVE> saves them.  The flag rides in the template
// argument, SIN_X = sine mode | INITQ_RAD, like DECODE_INITQ in decode_kernel: the inference instantiations keep their symbols.
constexpr int INITQ_RAD = 4;
// INITQ_ROWS512 (decoder mode 1 with init_q: K.1..3 are [256 x 256], the feature halves of Wx_1..3 do not exist and the body image
// holds zeros there): pass 2 computes Wx_0 alone, ONE M-tile pair per wave (channels 64 wave .. 64 wave + 63) in place of four, and
// channels 256..1023 of the record are NOT written -- pixel_chain_kernel<BK_SEEDS = true> seeds layers 1..3 from bK_i of the body
// image and writes k_i there.  Channels 0..255 and 1024..1279 hold the bits of the 1280-row form (the same gemm_pair, the same k
// order).  Rides in SIN_X as well; inference only.
constexpr int INITQ_ROWS512 = 8;
template <int SIN_X>
__global__ __launch_bounds__(256, 1) void initq_planes_kernel(const InitqParams p) {
    constexpr int SIN_MODE = SIN_X & (INITQ_RAD - 1);
    constexpr bool RAD = (SIN_X & INITQ_RAD) != 0;
    constexpr bool ROWS512 = (SIN_X & INITQ_ROWS512) != 0;
    static_assert(SIN_X >= 0 && SIN_X < 2 * INITQ_ROWS512 && !(RAD && ROWS512), "sine mode | INITQ_RAD or sine mode | INITQ_ROWS512");
    __shared__ __attribute__((aligned(16))) float buf[IQ_BUF];
    __shared__ __attribute__((aligned(16))) float tr[4][32 * IQ_TR_PITCH];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int b = blockIdx.z;
    const int bx0 = blockIdx.x * IQ_TW, by0 = p.y0 + blockIdx.y * IQ_TH;
    const int rows = p.y1 - p.y0;

    // ---- the B operand.  Slot (kk, nt, lane) = buf[(2 kk + nt) * 64 + lane] belongs to thread 64 (2 (kk & 1) + nt) + lane, so
    // a thread fills the slots of ONE pixel: N-tile nt = wave & 1, pixel j, lane half h, k-steps kk = 2 i + (wave >> 1).
    // Slot (kk, h) is unfolded channel n = c * 9 + tap with tap = kk / 32, c = 2 (kk % 32) + h (WP's k order).
    const int f_nt = wave & 1, f_kp = wave >> 1;
    int f_iy, f_ix;
    float relh, relw;
    {
        const int x = bx0 + (j & (IQ_TW - 1)), y = by0 + 4 * f_nt + (j >> 3);
        const int xc = x < p.Wu ? x : p.Wu - 1;            // pixels past the band compute on its last row / column (never stored)
        const int yc = y < p.y1 ? y : p.y1 - 1;
        axis_eval(p.ah, yc, f_iy, relh);
        axis_eval(p.aw, xc, f_ix, relw);
    }
    const float* __restrict__ F = p.iq + IQ_OFF_F;
#pragma unroll 4
    for (int i = 0; i < IQ_ITERS; ++i) {
        const int kk = 2 * i + f_kp;
        const int n = (2 * (kk & 31) + h) * 9 + (kk >> 5);
        float a = __builtin_fmaf(F[2 * UNF + n], p.ratio, F[3 * UNF + n]);
        a = __builtin_fmaf(F[1 * UNF + n], relw, a);
        a = __builtin_fmaf(F[0 * UNF + n], relh, a);
        if constexpr (RAD) buf[i * 256 + threadIdx.x] = dsin<SIN_MODE>(a);
        else buf[i * 256 + threadIdx.x] = dsin_rev<SIN_MODE>(a);
    }

    // where this lane's two store pixels of each N-tile go: transposed reads hand lane L pixel (L >> 2) + 16 i, chunk L & 3
    float* dst[2][2];
    bool dok[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pp = (lane >> 2) + 16 * i;
            const int x = bx0 + (pp & (IQ_TW - 1)), y = by0 + 4 * nt + (pp >> 3);
            dok[nt][i] = (x < p.Wu) && (y < p.y1);
            const int xs = dok[nt][i] ? x : 0, ys = dok[nt][i] ? y - p.y0 : 0;
            dst[nt][i] = p.pix + (((size_t)b * rows + ys) * p.Wu + xs) * PIX_CH + 4 * (lane & 3);
        }
    float* const trw = tr[wave];
    const int lane_off = lane * 16;
    constexpr int PF = P_PREFETCH;
    static_assert(WP_KG % PF == 0, "ring index must be static");

    // one M-tile pair (64 output channels from ch0) against both N-tiles: weight pieces from `wrs` at byte offset wp
    auto gemm_pair = [&](const __amdgpu_buffer_rsrc_t wrs, const int wp, const float* __restrict__ seed, const unsigned nanm,
                         const int ch0) {
        // the B operands do not depend on the pair: hide the base from LICM, or the LDS reads are hoisted out of the pair loop
        int off = lane;
        asm volatile("" : "+v"(off));
        const float* bm = buf + off;
        f32x4 r0v[PF], r1v[PF];
#pragma unroll
        for (int d = 0; d < PF; ++d) {
            r0v[d] = ld_piece(wrs, lane_off, wp + (2 * d + 0) * PIECE_BYTES);
            r1v[d] = ld_piece(wrs, lane_off, wp + (2 * d + 1) * PIECE_BYTES);
        }
        f32x16 a00, a01, a10, a11;                               // [N-tile][M-tile of the pair]
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 s0 = or_bits(*(const f32x4*)(seed + 4 * h + 8 * g), nanm);
            const f32x4 s1 = or_bits(*(const f32x4*)(seed + 32 + 4 * h + 8 * g), nanm);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a00[4 * g + e] = s0[e]; a10[4 * g + e] = s0[e];
                a01[4 * g + e] = s1[e]; a11[4 * g + e] = s1[e];
            }
        }
#pragma unroll
        for (int kg = 0; kg < WP_KG; ++kg) {
            const f32x4 u0 = r0v[kg % PF], u1 = r1v[kg % PF];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = 4 * kg + e;
                const float b0 = bm[(2 * kk + 0) * 64], b1 = bm[(2 * kk + 1) * 64];
                a00 = MFMA32(u0[e], b0, a00);
                a01 = MFMA32(u1[e], b0, a01);
                a10 = MFMA32(u0[e], b1, a10);
                a11 = MFMA32(u1[e], b1, a11);
            }
            if (kg + PF < WP_KG) {
                r0v[kg % PF] = ld_piece(wrs, lane_off, wp + (2 * (kg + PF) + 0) * PIECE_BYTES);
                r1v[kg % PF] = ld_piece(wrs, lane_off, wp + (2 * (kg + PF) + 1) * PIECE_BYTES);
            }
        }
        // transpose and store: 16 channels x 32 pixels at a time (LDS operations of a wave complete in issue order)
        auto put = [&](const f32x16& a, const int nt, const int chan) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int gg = 0; gg < 2; ++gg) {
                    const int g = 2 * half + gg;
                    *(f32x4*)(trw + j * IQ_TR_PITCH + 4 * (2 * gg + h)) = f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int pp = (lane >> 2) + 16 * i;
                    const f32x4 v = *(const f32x4*)(trw + pp * IQ_TR_PITCH + 4 * (lane & 3));
                    if (dok[nt][i]) {
                        f32x4* d = (f32x4*)(dst[nt][i] + chan + 16 * half);
                        if (p.stream_stores) __builtin_nontemporal_store(v, d);
                        else *d = v;
                    }
                }
            }
        };
        put(a00, 0, ch0);
        put(a01, 0, ch0 + 32);
        put(a10, 1, ch0);
        put(a11, 1, ch0 + 32);
    };

    __syncthreads();                                             // E is in LDS
    {
        const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)p.iq, 0, (int)(IQ_FLOATS * sizeof(float)), 0x00020000);   // reads past the end return 0
        // an image without its validity word answers NaN in every sine argument
        const unsigned nanm = __builtin_bit_cast(unsigned, p.iq[IQ_OFF_BQ0 + HID]) == (RAD ? DIINN_INITQ_TRAIN_MAGIC : DIINN_INITQ_MAGIC) ? 0u : 0x7fc00000u;
        gemm_pair(qrs, (int)(IQ_OFF_Q0W * sizeof(float)) + wave * (WP_KG * 2 * PIECE_BYTES), p.iq + IQ_OFF_BQ0 + 64 * wave, nanm,
                  PCH + 64 * wave);
    }
    __syncthreads();                                             // every wave has read E

    // ---- pass 2: x' = E * X[cell] in place; X[c * 9 + tap] = feat[b, c, iy + ky - 1, ix + kx - 1], zero outside the map
    {
        const float* __restrict__ fb = p.feat + (size_t)b * C_IN * p.H * p.W;
#pragma unroll 8
        for (int i = 0; i < IQ_ITERS; ++i) {
            const int kk = 2 * i + f_kp;
            const int tap = kk >> 5, c = 2 * (kk & 31) + h;
            const int ky = tap / 3, kx = tap - 3 * ky;
            const int yy = f_iy + ky - 1, xx = f_ix + kx - 1;
            const bool ok = (yy >= 0) && (yy < p.H) && (xx >= 0) && (xx < p.W);
            // unconditional load from a clamped address, then select (precompute_P_kernel says why)
            const int yc = yy < 0 ? 0 : (yy >= p.H ? p.H - 1 : yy);
            const int xc = xx < 0 ? 0 : (xx >= p.W ? p.W - 1 : xx);
            const float v = fb[((size_t)c * p.H + yc) * p.W + xc];
            buf[i * 256 + threadIdx.x] *= ok ? v : 0.0f;
        }
    }
    __syncthreads();                                             // E * X is in LDS
    {
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)p.Wt, 0, (int)(PACKED_FLOATS * sizeof(float)), 0x00020000);
        if constexpr (ROWS512) {
            gemm_pair(wrs, (int)(OFF_WP * sizeof(float)) + wave * (WP_KG * 2 * PIECE_BYTES), p.Wt + OFF_BK + 64 * wave, 0u, 64 * wave);
        } else {
#pragma unroll 1
            for (int mp = 4 * wave; mp < 4 * wave + 4; ++mp)
                gemm_pair(wrs, (int)(OFF_WP * sizeof(float)) + mp * (WP_KG * 2 * PIECE_BYTES), p.Wt + OFF_BK + 64 * mp, 0u, 64 * mp);
        }
    }
}

int launch_initq_planes(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                        float* pix_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode, bool rad, bool rows512) {
    if (rad && rows512) return DIINN_ERR_UNSUPPORTED;
    if (int st = check_band_args(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, initq_dev, pix_dev)) return st;
    const dim3 grid(grid_blocks(0, Wu, IQ_TW), grid_blocks(y0, y1, IQ_TH), B);
    if (int st = check_grid(grid.y, B)) return st;
    InitqParams p;
    p.feat = feat_dev; p.Wt = packed_dev; p.iq = initq_dev; p.pix = pix_dev;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu; p.y0 = y0; p.y1 = y1;
    p.ratio = (float)(((double)H * (double)W) / ((double)Hu * (double)Wu));
    const int small = diinn_uses_small_output_kernel(Hu, Wu);
    p.ah = make_axis(H, Hu, small);
    p.aw = make_axis(W, Wu, small);
    // streaming stores once the planes no longer fit beside anything in the 256 MiB last-level cache (launch_P's rule)
    p.stream_stores = (double)B * (y1 - y0) * Wu * PIX_CH * 4.0 >= 128.0 * 1024 * 1024;
    return launch_sin<INITQ_RAD, INITQ_ROWS512, 0>(sin_mode, rad ? INITQ_RAD : rows512 ? INITQ_ROWS512 : 0, [&](auto S, auto F) {
        hipLaunchKernelGGL(initq_planes_kernel<decltype(S)::value | decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

extern "C" int diinn_initq_planes(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                  float* pix_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return launch_initq_planes(stream, feat_dev, packed_dev, initq_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false);
}

// decoder mode 1 with init_q: channels 0..255 and 1024..1279 only (INITQ_ROWS512)
extern "C" int diinn_initq_planes_m1(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                     float* pix_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return launch_initq_planes(stream, feat_dev, packed_dev, initq_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false, true);
}
