// diinn_pixel_chain_x3.hip -- decoder init_q=True, modes 1 and 2: the per-pixel modulation chain in split-bf16 arithmetic
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, image and plane layout in diinn_layout.h)
//
// pixel_chain_kernel's contract (diinn_decode.hip) on the arithmetic of DIINN_COMPUTE_BF16X3: the pixel records
// [B][rows][Wu][PIX_CH] of initq_planes_x3_kernel are updated in place,
//   k_0 = relu(PIX[0:256]),   k_i = relu(K_i[:, :256] . k_{i-1} + seed_i),  i = 1..3,   fp32 k_i -> channels 256 i .. 256 i + 255
// with seed_i the slot itself (mode 2) or, BK_SEEDS, bK_i of section BK of the body image (mode 1: the 512-row planes leave the
// slots unwritten).  Channels 0..255 and 1024..1279 are read (0..255) or left alone and never written.
// decode_bf16x3_kernel<SIN | X3_INITQ | X3_QONLY> (diinn_bf16x3.hip) reads k_i there as the multiplier of the sine.
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// pixel_chain_x3_kernel: three [256 x 256] . [256 x pixels] products per pixel on v_mfma_f32_32x32x16_bf16.  Every operand is carried
// as hi = bf16(v), lo = bf16(v - hi); the three terms of a k-step go to ONE fp32 accumulator in the library's order -- w_lo.k_hi,
// w_hi.k_lo, w_hi.k_hi -- and the accumulator starts from seed_i.  k_{i-1} is split in registers from the fp32 value just computed
// (k_0 from the rectified record), so what the next layer multiplies is the split of exactly what the record holds.
// Weights: pieces 0 and 2 (k_hi, k_lo) of each k-step of section WLX, in WLX's k order (chan_of_bf16), through a register ring of
// those two pieces -- the Q-only form of decode_bf16x3_kernel streams pieces 1 and 3 of the same k-steps the same way.  No image of
// its own.  A body image without its derived sections answers NaN (derived_nan_mask, folded into every seed).
//
// Layout: decode_bf16x3_kernel's park-slab scheme, not chain_body's register-to-register one.  One wave owns 32 pixels (an 8 x 4
// tile; workgroup = 4 waves = 16 x 8 pixels, pixel_chain_kernel's grid); lane (h, j) holds pixel j's B fragments, and accumulator
// registers 8 s .. 8 s + 7 of M-tile m ARE fragment 2 m + s of the next layer, so nothing crosses lanes.  The activation is 16
// fragments hi + 16 lo = 128 registers; chain_body keeps k_i and k_{i+1} both in registers (2 x 128 fp32), which in this arithmetic
// would be 256 registers of fragments beside accumulators, ring and seeds.  The next layer's fragments are parked in a wave-private
// LDS slab instead (32 KiB per wave; a lane re-reads only what it wrote: no barrier, no __syncthreads in the kernel).
// Occupancy it is designed for: ONE wave per SIMD (one workgroup of four waves per CU: 128 KiB of LDS, up to 512 registers).
// The epilogue of M-tile m - 1 (relu, the fp32 store, the split) runs one element per k-step under M-tile m's MFMAs, as in
// decode_bf16x3_kernel.  The record stores and the weight loads share the wave's one memory counter (initq_planes_x3_kernel's header),
// so the ring is EIGHT k-steps deep here, 768 MFMA clocks: a weight wait behind a store burst finds the stores retired.
//
// Roofline, from counting: per pixel 1 KiB (mode 1) or 4 KiB (mode 2) read and 3 KiB written, against 3 x 3 x 2 x 256 x 256 =
// 1.18 MFLOP on the bf16 MFMA.  Per wave and layer 384 MFMAs of 32 clocks: 36,864 clocks per 32 pixels and SIMD, 0.49 ms for the
// 2^20 pixels of a 1024 x 1024 output on 1,024 SIMDs at 2.4 GHz; the same pixels move 7 GiB, 1.5 ms and more of HBM time when the
// planes do not stay in the last-level cache.  Memory sets the pace, not the matrix cores (DESIGN.md 3.6e has what was measured).
//
// A lane past the edge computes on a record of its own wave (the clamped pixel lies in the wave's tile) and stores nothing.  A
// pixel's arithmetic depends on the pixel alone: any split of the rows into launches gives the same bits.  No atomics, no scratch.
// ---------------------------------------------------------------------------------
struct PixChainX3Params {
    float* pix;          // [B][rows][Wu][PIX_CH]: the pixel planes of one chunk of HR rows
    const float* Wt;     // body image (sections WLX, BK)
    int B, Wu, rows;
};

constexpr int PCX_PF = 8;                                   // ring depth in k-steps (2 pieces, 3 MFMAs each)

// issue order of a k-step: a weight load behind each of the first two MFMAs, the epilogue's VALU spread over the three; the region
// ends at the k-step (X3_KSTEP_ORDER_Q of diinn_bf16x3.hip)
#define PCX_KSTEP_ORDER()                                                             \
    do {                                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < 3; ++i_) {                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        \
            if (i_ < 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);            \
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                        \
        }                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                            \
    } while (0)

template <bool BK_SEEDS>
__global__ __launch_bounds__(256, 1) void pixel_chain_x3_kernel(const PixChainX3Params p) {
    __shared__ __attribute__((aligned(16))) bf16x8 park[4][2][16][64];     // [wave][hi, lo][fragment][lane] = 128 KiB
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int x = blockIdx.x * (TILE_W * WG_TILES_X) + (wave & 1) * TILE_W + (j & (TILE_W - 1));
    const int y = blockIdx.y * (TILE_H * WG_TILES_Y) + (wave >> 1) * TILE_H + (j / TILE_W);
    const int b = blockIdx.z;
    const bool valid = (x < p.Wu) && (y < p.rows);
    if (__builtin_amdgcn_readfirstlane((int)(__ballot(valid) == 0ull))) return;
    const int xc = x < p.Wu ? x : p.Wu - 1;
    const int yc = y < p.rows ? y : p.rows - 1;
    float* __restrict__ Pc = p.pix + (((size_t)b * p.rows + yc) * p.Wu + xc) * PIX_CH + 4 * h;
    const float* __restrict__ Wt = p.Wt;
    const unsigned nanm = derived_nan_mask(Wt);

    // ---- k_0 = relu(PIX[0:256]), split into hi/lo fragments: channel 32 m + 8 g + 4 h + e -> fragment 2 m + (g >> 1), element 4 (g & 1) + e
    bf16x8 qh[16], ql[16];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 pv = *(const f32x4*)(Pc + 32 * m + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                __bf16 vh, vl;
                split_bf16(relu0(pv[e]), vh, vl);
                qh[2 * m + (g >> 1)][4 * (g & 1) + e] = vh;
                ql[2 * m + (g >> 1)][4 * (g & 1) + e] = vl;
            }
        }
    }

    constexpr int PF = PCX_PF;
    static_assert(16 % PF == 0, "ring index must be static");
    constexpr int KS_BYTES = (int)(WLX_KSTEP * sizeof(float));
    // (the ring's eight k-steps past the last layer's end land in section WPX: inside the image, never used)
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)Wt, 0, (int)(PACKED_FLOATS * sizeof(float)), 0x00020000);
    const int lane_off = lane * 16;
    // pieces 0 and 2 of a k-step (k_hi, k_lo) by immediate offsets from one scalar offset
    auto ld_kstep = [&](f32x4& kh, f32x4& kl, const int soff) {
        kh = ld_piece(wrs, lane_off, soff);
        kl = ld_piece(wrs, lane_off + 2 * PIECE_BYTES, soff);
    };
    int wp = (int)(OFF_WLX * sizeof(float));
    f32x4 rkh[PF], rkl[PF];
#pragma unroll
    for (int d = 0; d < PF; ++d) ld_kstep(rkh[d], rkl[d], wp + d * KS_BYTES);
    // seed_i of M-tile m: channels 32 m + 8 g + 4 h ..
    auto seeds = [&](const int layer, const int m, const int g) -> f32x4 {
        if constexpr (BK_SEEDS) return *(const f32x4*)(Wt + OFF_BK + (layer + 1) * HID + 4 * h + 32 * m + 8 * g);
        else return *(const f32x4*)(Pc + (layer + 1) * HID + 32 * m + 8 * g);
    };
    f32x4 sk[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) sk[g] = seeds(0, 0, g);
    bf16x8 (*mine)[16][64] = park[wave];

#pragma unroll 1
    for (int layer = 0; layer < 3; ++layer) {
        const int nl = layer < 2 ? layer + 1 : 2;
        float* Pl = Pc + (layer + 1) * HID;
        f32x16 pk;
        bf16x8 fh, fl;
        f32x4 fq;
        // element r of M-tile mt (channel 32 mt + 8 (r >> 2) + 4 h + (r & 3)): rectified, stored as fp32 four at a time, split and parked
        auto finish = [&](const int mt, const int r, const float kraw) {
            float v = relu0(kraw);
            asm volatile("" : "+v"(v));                           // the element stays behind its k-step (see decode_bf16x2_kernel)
            fq[r & 3] = v;
            if ((r & 3) == 3 && valid) *(f32x4*)(Pl + 32 * mt + 8 * (r >> 2)) = fq;
            __bf16 vh, vl;
            split_bf16(v, vh, vl);
            fh[r & 7] = vh;
            fl[r & 7] = vl;
            if ((r & 7) == 7) {
                mine[0][2 * mt + (r >> 3)][lane] = fh;
                mine[1][2 * mt + (r >> 3)][lane] = fl;
            }
        };
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            f32x16 ak;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 s0 = or_bits(sk[g], nanm);
#pragma unroll
                for (int e = 0; e < 4; ++e) ak[4 * g + e] = s0[e];
            }
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                const int s = m * 16 + ks;
                const bf16x8 wkh = __builtin_bit_cast(bf16x8, rkh[s % PF]);
                // the two small products first, the leading one last
                ak = MFMA_BF16(__builtin_bit_cast(bf16x8, rkl[s % PF]), qh[ks], ak);
                ak = MFMA_BF16(wkh, ql[ks], ak);
                ak = MFMA_BF16(wkh, qh[ks], ak);
                ld_kstep(rkh[s % PF], rkl[s % PF], wp + (s + PF) * KS_BYTES);
                if (ks == 2) {                                    // the next M-tile's seeds (after the last: the next layer's first)
#pragma unroll
                    for (int g = 0; g < 4; ++g) sk[g] = m < 7 ? seeds(layer, m + 1, g) : seeds(nl, 0, g);
                }
                if (m > 0) finish(m - 1, ks, pk[ks]);             // one epilogue element of tile m - 1 per k-step
                PCX_KSTEP_ORDER();
            }
            pk = ak;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) finish(7, r, pk[r]);
        // the parked activation becomes the next layer's B operand (after the last layer: read and dropped)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            qh[i] = mine[0][i][lane];
            ql[i] = mine[1][i][lane];
        }
        wp += (int)(WLX_LAYER * sizeof(float));
    }
}

// diinn_pixel_chain's checks (pixel_chain_impl, diinn_decode.hip), then the launch
int launch_pixel_chain_x3(void* stream, float* pix_dev, const float* packed_dev, int B, int Wu, int rows, bool bk_seeds) {
    if (!all_set(pix_dev, packed_dev)) return DIINN_ERR_INVALID_ARG;
    if (B <= 0 || Wu <= 0 || rows <= 0) return DIINN_ERR_INVALID_ARG;
    if ((((size_t)pix_dev) | ((size_t)packed_dev)) & 15) return DIINN_ERR_INVALID_ARG;      // 16-byte seeds and pieces
    if (int st = check_extent(rows, Wu)) return st;
    const dim3 grid(grid_blocks(0, Wu, WG_W), grid_blocks(0, rows, WG_H), B);
    if (int st = check_grid(grid.y, B)) return st;
    const PixChainX3Params p{pix_dev, packed_dev, B, Wu, rows};
    pick<1, 0>(bk_seeds, [&](auto S) {
        hipLaunchKernelGGL(pixel_chain_x3_kernel<decltype(S)::value>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
    return hip_status(hipGetLastError());
}

extern "C" int diinn_pixel_chain_x3(void* stream, float* pix_dev, const float* packed_dev, int B, int Wu, int rows, int bk_seeds) {
    return launch_pixel_chain_x3(stream, pix_dev, packed_dev, B, Wu, rows, bk_seeds != 0);
}
