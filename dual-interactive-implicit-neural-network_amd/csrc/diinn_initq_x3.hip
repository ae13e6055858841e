// diinn_initq_x3.hip -- decoder init_q=True, mode 3: the pixel planes of diinn_initq.hip in split-bf16 arithmetic
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, image and plane layout in diinn_layout.h)
//
// The same record per HR pixel as initq_planes_kernel writes, fp32:
//   PIX[0..1023]    = Wx . x' + bK            x' = E * X[cell],  E = sin(first_layer . (rel_h, rel_w, ratio) + bF)
//   PIX[1024..1279] = (Q0 . E + bQ0) / (2 pi)
// with both GEMMs in the arithmetic of DIINN_COMPUTE_BF16X3: every operand v is carried as hi = bf16(v),
// lo = bf16(v - hi) and a product is w_lo.x_hi + w_hi.x_lo + w_hi.x_hi on v_mfma_f32_32x32x16_bf16, fp32 accumulation, the three
// terms of a k-step added to the accumulator in that order (as precompute_P_x3_kernel and decode_bf16x3_kernel add them).
// decode_bf16x3_kernel<SIN | X3_INITQ> (diinn_bf16x3.hip) runs the layers and the head from these planes.
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// initq_planes_x3_kernel: a GEMM [1280 x 576] . [576 x pixels] on the bf16 MFMA, from initq_planes_kernel's structure.
// Workgroup = 8 waves = an 8 x 8 tile of HR pixels = two N-tiles of 8 x 4, TWO waves per SIMD.  The hi / lo B operand of the whole
// tile lives in ONE LDS buffer [k-step 36][hi, lo][N-tile 2][lane 64] of 16-byte fragments (144 KiB of the CU's 160), filled twice:
//   pass 1  hi/lo(E): E by the fp32 kernel's sequence -- fma(F2, ratio, bF), then rel_w, then rel_h, then dsin_rev<SIN_MODE> --
//           -> every wave runs ONE M-tile of Q0 (the init_q SPLIT image) on both N-tiles: channels 1024 + 32 wave ..
//   pass 2  hi/lo(x') in place, x' = (E_hi + E_lo) * X in fp32 (THE IN-PLACE FORM: only the parts of E survive pass 1, which
//           adds 2^-18 |x'| to the split's own 2^-17; each thread owns the fragments it wrote; X by clamped loads and a select)
//           -> every wave runs two M-tile pairs of Wx (section WPX of the body image): channels 128 wave .. 128 wave + 127.
// k-step s = 9 group + tap covers unfolded channels n = c * 9 + tap, c = 16 group + 8 (lane >> 5) + j (WPX's k order; the init_q
// split image is packed in the same order, so one B fragment serves both GEMMs).  A wave keeps both N-tiles' accumulators of its
// M-tiles: the four 1 KiB pieces of a k-step (M-tile 0 hi, lo, M-tile 1 hi, lo: contiguous in both images) feed 12 MFMAs, its
// four B fragments are four ds_read_b128 at immediate offsets.  Results leave through a per-wave LDS transpose, 16 channels of
// 16 pixels at a time, so that four lanes write 64 contiguous bytes of a pixel's record.
// Why two waves per SIMD (measured): the record stores and the weight loads share the wave's one memory counter,
// so the first weight wait after a tile's stores waits for the stores as well -- with one wave per SIMD the matrix core idles
// through every store burst (178 of 344 us per chunk); the second wave computes meanwhile.
// A pixel's arithmetic depends on nothing but the pixel: bands and chunks of rows are bit-identical to the whole image, and
// channels 1024..1279 do not depend on the batch item.  No atomics, no scratch, one workgroup per CU.
// ---------------------------------------------------------------------------------
struct InitqX3Params {
    const float* feat;   // [B,64,H,W]
    const float* Wt;     // body image (sections WPX, BK)
    const float* iq;     // init_q image (F); INITQ_X3_RAD: the init_q training image (F, BQ0 in radians)
    const float* iqx;    // init_q split image (diinn_pack_initq_x3); INITQ_X3_RAD: the init_q split training image (WX, Q0X)
    float* pix;          // [B][y1 - y0][Wu][PIX_CH]
    int B, H, W, Hu, Wu, y0, y1;
    float ratio;         // fp32(H*W / (Hu*Wu))   (diinn.py:166)
    Axis ah, aw;
    int stream_stores;   // the planes are larger than the last-level cache: write them with streaming (nt) stores
};

constexpr int IX_TW = 8, IX_TH = 8;                       // HR pixels per workgroup: two N-tiles of 8 x 4
constexpr int IX_WAVES = 8;
constexpr int IX_KS = WPB_KS;                             // 36 k-steps of 16 unfolded channels
constexpr int IX_TR_PITCH = 20;                           // floats per pixel in the store transpose (16 + 4)
constexpr int IX_STEP_BYTES = 4 * PIECE_BYTES;            // the four weight pieces of a k-step
constexpr int IX_PAIR_BYTES = IX_KS * IX_STEP_BYTES;      // an M-tile pair's weights: 144 KiB
constexpr int IX_PF = 4;                                  // weight ring depth in k-steps

// INITQ_X3_RAD (the split training forward, diinn_decode_initq_train_fwd_x3): the radians form, as INITQ_RAD is initq_planes_kernel's.
// `iq` is the init_q TRAINING image (F and BQ0 in radians, DIINN_INITQ_TRAIN_MAGIC), `iqx` the init_q SPLIT TRAINING image
// (diinn_layout.h: WX in section WPX's order, Q0X in the init_q split image's, nothing divided by 2 pi, its own validity word), so
// E = dsin<SIN_MODE>(a) takes a in radians, BOTH GEMMs stream from `iqx` -- the training body image has no section WPX -- and
// channels 1024..1279 leave as Q0 . E + bQ0 in radians, as decode_bf16x3_kernel<SIN | X3_INITQ | X3_SAVE> saves them.  Launched over
// the whole image.  The flag rides in the template argument, SIN_X = sine mode | INITQ_X3_RAD: the inference instantiations keep
// their symbols and their instructions.
constexpr int INITQ_X3_RAD = 4;
// INITQ_X3_ROWS512 (decoder mode 1 with init_q, as INITQ_ROWS512 is initq_planes_kernel's: K.1..3 are [256 x 256], the feature halves
// of Wx_1..3 do not exist): pass 1 is unchanged; pass 2 computes Wx_0 alone -- its four M-tile pairs as eight M-tiles, ONE per wave
// (channels 32 wave .. 32 wave + 31, the hi / lo pieces of M-tile wave & 1 of pair wave >> 1) -- and channels 256..1023 of the record
// are NOT written: pixel_chain_x3_kernel<BK_SEEDS = true> seeds layers 1..3 from bK_i and writes k_i there.  Channels 0..255 and
// 1024..1279 hold the bits of the 1280-row form: an output channel's terms and their order do not depend on how many M-tiles share
// the B fragments.  Rides in SIN_X as well, not combinable with INITQ_X3_RAD; inference only.
constexpr int INITQ_X3_ROWS512 = 8;
template <int SIN_X>
__global__ __launch_bounds__(64 * IX_WAVES) void initq_planes_x3_kernel(const InitqX3Params p) {
    constexpr int SIN_MODE = SIN_X & (INITQ_X3_RAD - 1);
    constexpr bool RAD = (SIN_X & INITQ_X3_RAD) != 0;
    constexpr bool ROWS512 = (SIN_X & INITQ_X3_ROWS512) != 0;
    static_assert(SIN_X >= 0 && SIN_X < 2 * INITQ_X3_ROWS512 && !(RAD && ROWS512) && SIN_MODE >= DIINN_SIN_ACCURATE && SIN_MODE <= DIINN_SIN_HW_REDUCED,
                  "sine mode | INITQ_X3_RAD or sine mode | INITQ_X3_ROWS512");
    __shared__ __attribute__((aligned(16))) bf16x8 buf[IX_KS][2][2][64];   // [k-step][hi, lo][N-tile][lane] = 144 KiB
    __shared__ __attribute__((aligned(16))) float tr[IX_WAVES][16 * IX_TR_PITCH];   // 10 KiB
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int b = blockIdx.z;
    const int bx0 = blockIdx.x * IX_TW, by0 = p.y0 + blockIdx.y * IX_TH;
    const int rows = p.y1 - p.y0;

    // ---- the B operand.  A thread fills fragments of ONE pixel, lane = pixel (N-tile lane >> 5, pixel lane & 31 of it), and a WAVE
    // fills one lane half f_h = wave & 1 of ONE channel group g = wave >> 1, all nine taps: the 8 x 9 unfolded channels
    // n = (16 g + 8 f_h + jj) * 9 + tap of a (group, half) are 72 consecutive floats of each row of F, and their addresses are the
    // same in every lane -- the first layer comes through the scalar cache.  Fragment element jj of k-step s = 9 g + tap is
    // channel 16 g + 8 f_h + jj at that tap.
    const int f_h = wave & 1, f_g = wave >> 1;
    int f_iy, f_ix;
    float relh, relw;
    {
        const int x = bx0 + (lane & (IX_TW - 1)), y = by0 + (lane >> 3);
        const int xc = x < p.Wu ? x : p.Wu - 1;            // pixels past the band compute on its last row / column (never stored)
        const int yc = y < p.y1 ? y : p.y1 - 1;
        axis_eval(p.ah, yc, f_iy, relh);
        axis_eval(p.aw, xc, f_ix, relw);
    }
    // fragment (tap, part) of this thread: fill[(2 tap + part) * 128]
    bf16x8* const fill = &buf[9 * f_g][0][0][0] + ((lane >> 5) * 64 + 32 * f_h + (lane & 31));
    {
        const float* __restrict__ F = p.iq + IQ_OFF_F + (16 * f_g + 8 * f_h) * 9;   // wave-uniform
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            bf16x8 eh, el;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int n = jj * 9 + tap;
                float a = __builtin_fmaf(F[2 * UNF + n], p.ratio, F[3 * UNF + n]);
                a = __builtin_fmaf(F[1 * UNF + n], relw, a);
                a = __builtin_fmaf(F[0 * UNF + n], relh, a);
                float e;
                if constexpr (RAD) e = dsin<SIN_MODE>(a); else e = dsin_rev<SIN_MODE>(a);
                const __bf16 hi = (__bf16)e;
                eh[jj] = hi;
                el[jj] = (__bf16)(e - (float)hi);
            }
            fill[(2 * tap + 0) * 128] = eh;
            fill[(2 * tap + 1) * 128] = el;
        }
    }

    // where this lane's store pixel of each (N-tile, half of its pixels) goes: transposed reads hand lane L pixel (L >> 2) + 16 i
    // of the N-tile, chunk L & 3
    float* dst[2][2];
    bool dok[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pp = (lane >> 2) + 16 * i;
            const int x = bx0 + (pp & (IX_TW - 1)), y = by0 + 4 * nt + (pp >> 3);
            dok[nt][i] = (x < p.Wu) && (y < p.y1);
            const int xs = dok[nt][i] ? x : 0, ys = dok[nt][i] ? y - p.y0 : 0;
            dst[nt][i] = p.pix + (((size_t)b * rows + ys) * p.Wu + xs) * PIX_CH + 4 * (lane & 3);
        }
    float* const trw = tr[wave];
    const int lane_off = lane * 16;
    static_assert(IX_KS % IX_PF == 0, "ring index must be static");

    // NM M-tiles (32 NM output channels from ch0) against both N-tiles: per k-step the 2 NM pieces (hi, lo per M-tile) from `wrs`
    // at byte offset wp, k-steps IX_STEP_BYTES apart
    auto gemm = [&](auto nm_tag, const __amdgpu_buffer_rsrc_t wrs, const int wp, const float* __restrict__ seed, const unsigned nanm,
                    const int ch0) {
        constexpr int NM = decltype(nm_tag)::value;
        // the B operands do not depend on the M-tiles: hide the base from LICM, or the LDS reads are hoisted out of the pair loop
        int off = lane;
        asm volatile("" : "+v"(off));
        const bf16x8* bm = &buf[0][0][0][0] + off;
        f32x4 r[IX_PF][2 * NM];                                  // [slot][M-tile 0 hi, lo (, M-tile 1 hi, lo)]
#pragma unroll
        for (int d = 0; d < IX_PF; ++d)
#pragma unroll
            for (int q = 0; q < 2 * NM; ++q) r[d][q] = ld_piece(wrs, lane_off + q * PIECE_BYTES, wp + d * IX_STEP_BYTES);
        f32x16 acc[2][NM];                                       // [N-tile][M-tile]
#pragma unroll
        for (int mt = 0; mt < NM; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 s0 = or_bits(*(const f32x4*)(seed + 32 * mt + 4 * h + 8 * g), nanm);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[0][mt][4 * g + e] = acc[1][mt][4 * g + e] = s0[e];
            }
#pragma unroll
        for (int s = 0; s < IX_KS; ++s) {
            const bf16x8 xh[2] = {bm[((2 * s + 0) * 2 + 0) * 64], bm[((2 * s + 0) * 2 + 1) * 64]};
            const bf16x8 xl[2] = {bm[((2 * s + 1) * 2 + 0) * 64], bm[((2 * s + 1) * 2 + 1) * 64]};
            // the two small products first, the leading one last
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < NM; ++mt)
                    acc[nt][mt] = MFMA_BF16(__builtin_bit_cast(bf16x8, r[s % IX_PF][2 * mt + 1]), xh[nt], acc[nt][mt]);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < NM; ++mt)
                    acc[nt][mt] = MFMA_BF16(__builtin_bit_cast(bf16x8, r[s % IX_PF][2 * mt + 0]), xl[nt], acc[nt][mt]);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < NM; ++mt)
                    acc[nt][mt] = MFMA_BF16(__builtin_bit_cast(bf16x8, r[s % IX_PF][2 * mt + 0]), xh[nt], acc[nt][mt]);
            if (s + IX_PF < IX_KS) {
#pragma unroll
                for (int q = 0; q < 2 * NM; ++q)
                    r[s % IX_PF][q] = ld_piece(wrs, lane_off + q * PIECE_BYTES, wp + (s + IX_PF) * IX_STEP_BYTES);
            }
            // the region ends at the k-step: without it hipcc sinks every ring load to its use (a wait for each, no prefetch)
            __builtin_amdgcn_sched_barrier(0);
        }
        // transpose and store: 16 channels x 16 pixels at a time (LDS operations of a wave complete in issue order)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < NM; ++mt)
#pragma unroll
                for (int half = 0; half < 2; ++half)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if ((j >> 4) == i) {
#pragma unroll
                            for (int gg = 0; gg < 2; ++gg) {
                                const int g = 2 * half + gg;
                                const f32x16& a = acc[nt][mt];
                                *(f32x4*)(trw + (j & 15) * IX_TR_PITCH + 4 * (2 * gg + h)) = f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
                            }
                        }
                        const f32x4 v = *(const f32x4*)(trw + (lane >> 2) * IX_TR_PITCH + 4 * (lane & 3));
                        if (dok[nt][i]) {
                            f32x4* d = (f32x4*)(dst[nt][i] + ch0 + 32 * mt + 16 * half);
                            if (p.stream_stores) __builtin_nontemporal_store(v, d);
                            else *d = v;
                        }
                    }
    };

    __syncthreads();                                             // hi/lo(E) is in LDS
    if constexpr (RAD) {
        const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)p.iqx, 0, (int)(IQS_FLOATS * sizeof(float)), 0x00020000);
        // a training image or a split training image without its validity word answers NaN in every sine argument
        const bool ok = __builtin_bit_cast(unsigned, p.iqx[IQS_OFF_WORD]) == DIINN_INITQ_SPLIT_TRAIN_MAGIC &&
                        __builtin_bit_cast(unsigned, p.iq[IQ_OFF_BQ0 + HID]) == DIINN_INITQ_TRAIN_MAGIC;
        const unsigned nanm = ok ? 0u : 0x7fc00000u;
        gemm(IC<1>{}, qrs, (int)(IQS_OFF_Q0X * sizeof(float)) + (wave >> 1) * IX_PAIR_BYTES + (wave & 1) * 2 * PIECE_BYTES,
             p.iq + IQ_OFF_BQ0 + 32 * wave, nanm, PCH + 32 * wave);
    } else {
        const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)p.iqx, 0, (int)(IQX_FLOATS * sizeof(float)), 0x00020000);   // reads past the end return 0
        // an init_q image or a split image without its validity word answers NaN in every sine argument
        const bool ok = __builtin_bit_cast(unsigned, p.iqx[IQX_OFF_BQ0 + HID]) == DIINN_INITQ_X3_MAGIC &&
                        __builtin_bit_cast(unsigned, p.iq[IQ_OFF_BQ0 + HID]) == DIINN_INITQ_MAGIC;
        const unsigned nanm = ok ? 0u : 0x7fc00000u;
        // M-tile `wave` of the 8: pair wave >> 1, its pieces (wave & 1) hi, lo
        gemm(IC<1>{}, qrs, (int)(IQX_OFF_Q0X * sizeof(float)) + (wave >> 1) * IX_PAIR_BYTES + (wave & 1) * 2 * PIECE_BYTES,
             p.iqx + IQX_OFF_BQ0 + 32 * wave, nanm, PCH + 32 * wave);
    }
    __syncthreads();                                             // every wave has read E

    // ---- pass 2: x' = E * X[cell] in place; X[c * 9 + tap] = feat[b, c, iy + ky - 1, ix + kx - 1], zero outside the map
    {
        const size_t fplane = (size_t)p.H * p.W;
        const float* __restrict__ src = p.feat + ((size_t)b * C_IN + 16 * f_g + 8 * f_h) * fplane;
        int ro[3], co[3];
        bool rok[3], cok[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int yy = f_iy + k - 1, xx = f_ix + k - 1;
            rok[k] = (yy >= 0) && (yy < p.H);
            cok[k] = (xx >= 0) && (xx < p.W);
            ro[k] = (yy < 0 ? 0 : (yy >= p.H ? p.H - 1 : yy)) * p.W;
            co[k] = xx < 0 ? 0 : (xx >= p.W ? p.W - 1 : xx);
        }
        // unconditional loads from clamped addresses, the select afterwards (precompute_P_kernel says why; the empty asm statements
        // behind ALL the loads keep hipcc from moving a load under its select's condition, where each is followed by its own wait)
        float xv[9][8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) xv[tap][jj] = src[(size_t)jj * fplane + ro[tap / 3] + co[tap % 3]];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) asm volatile("" : "+v"(xv[tap][jj]));
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bool ok = rok[tap / 3] && cok[tap % 3];
            const bf16x8 eh = fill[(2 * tap + 0) * 128], el = fill[(2 * tap + 1) * 128];
            bf16x8 xh, xl;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float e = (float)eh[jj] + (float)el[jj];   // exact: the two parts of E
                const float xp = e * (ok ? xv[tap][jj] : 0.0f);
                const __bf16 hi = (__bf16)xp;
                xh[jj] = hi;
                xl[jj] = (__bf16)(xp - (float)hi);
            }
            fill[(2 * tap + 0) * 128] = xh;
            fill[(2 * tap + 1) * 128] = xl;
        }
    }
    __syncthreads();                                             // hi/lo(E * X) is in LDS
    if constexpr (RAD) {                                         // Wx from the split training image; bK from the body image (a permutation section)
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)p.iqx, 0, (int)(IQS_FLOATS * sizeof(float)), 0x00020000);
#pragma unroll 1
        for (int mp = 2 * wave; mp < 2 * wave + 2; ++mp)
            gemm(IC<2>{}, wrs, (int)(IQS_OFF_WX * sizeof(float)) + mp * IX_PAIR_BYTES, p.Wt + OFF_BK + 64 * mp, 0u, 64 * mp);
    } else {
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)p.Wt, 0, (int)(PACKED_FLOATS * sizeof(float)), 0x00020000);
        const unsigned nanm = derived_nan_mask(p.Wt);            // a body image without its derived sections (WPX) answers NaN
        if constexpr (ROWS512) {                                 // M-tile `wave` of Wx_0's eight: pair wave >> 1, its pieces (wave & 1) hi, lo
            gemm(IC<1>{}, wrs, (int)(OFF_WPX * sizeof(float)) + (wave >> 1) * IX_PAIR_BYTES + (wave & 1) * 2 * PIECE_BYTES,
                 p.Wt + OFF_BK + 32 * wave, nanm, 32 * wave);
        } else {
#pragma unroll 1
            for (int mp = 2 * wave; mp < 2 * wave + 2; ++mp)
                gemm(IC<2>{}, wrs, (int)(OFF_WPX * sizeof(float)) + mp * IX_PAIR_BYTES, p.Wt + OFF_BK + 64 * mp, nanm, 64 * mp);
        }
    }
}

int launch_initq_planes_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                           const float* initq_x3_dev, float* pix_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1,
                           int sin_mode, bool rad, bool rows512) {
    if (rad && rows512) return DIINN_ERR_UNSUPPORTED;
    if (int st = check_band_args(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev)) return st;
    const dim3 grid(grid_blocks(0, Wu, IX_TW), grid_blocks(y0, y1, IX_TH), B);
    if (int st = check_grid(grid.y, B)) return st;
    InitqX3Params p;
    p.feat = feat_dev; p.Wt = packed_dev; p.iq = initq_dev; p.iqx = initq_x3_dev; p.pix = pix_dev;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu; p.y0 = y0; p.y1 = y1;
    p.ratio = (float)(((double)H * (double)W) / ((double)Hu * (double)Wu));
    const int small = diinn_uses_small_output_kernel(Hu, Wu);
    p.ah = make_axis(H, Hu, small);
    p.aw = make_axis(W, Wu, small);
    // streaming stores once the planes no longer fit beside anything in the 256 MiB last-level cache (launch_P's rule)
    p.stream_stores = (double)B * (y1 - y0) * Wu * PIX_CH * 4.0 >= 128.0 * 1024 * 1024;
    return launch_sin<0, INITQ_X3_RAD, INITQ_X3_ROWS512>(sin_mode, rad ? INITQ_X3_RAD : rows512 ? INITQ_X3_ROWS512 : 0, [&](auto S, auto F) {
        hipLaunchKernelGGL(initq_planes_x3_kernel<decltype(S)::value | decltype(F)::value>, grid, dim3(64 * IX_WAVES), 0, (hipStream_t)stream, p);
    });
}

extern "C" int diinn_initq_planes_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                     const float* initq_x3_dev, float* pix_dev, int B, int H, int W, int Hu, int Wu, int y0,
                                     int y1, int sin_mode) {
    return launch_initq_planes_x3(stream, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false);
}

// decoder mode 1 with init_q: channels 0..255 and 1024..1279 only (INITQ_X3_ROWS512)
extern "C" int diinn_initq_planes_m1_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                        const float* initq_x3_dev, float* pix_dev, int B, int H, int W, int Hu, int Wu, int y0,
                                        int y1, int sin_mode) {
    return launch_initq_planes_x3(stream, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false, true);
}
