// diinn_liif_x3.hip -- the optional split-bf16 form of the LIIF comparison decoder (LIIF.hip_split_bf16)
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h)
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// liif_x3_kernel: liif_kernel<false> (diinn_baselines.hip) with the three 256 x 256 ReLU layers of every ensemble member on
// v_mfma_f32_32x32x16_bf16 in the split arithmetic of decode_bf16x3_kernel's Q-only form (diinn_bf16x3.hip): every operand is
// carried as hi = bf16(v), lo = bf16(v - hi), and a product is  w_lo . h_hi + w_hi . h_lo + w_hi . h_hi  on ONE fp32 accumulator
// seeded with the layer's bias -- three bf16 MFMAs (96 clocks) for the eight fp32 MFMAs (512 clocks) of a k-step of 16 channels.
//   * grid, pixel ownership, liif_axis_eval, the four areas, the early exit and the clamped lanes: liif_kernel<false>'s code;
//   * layer 1 in fp32, liif_kernel's expression bit for bit on the fp32 hoisted conv P; its register order q[16 m + r] IS the
//     B-fragment order (registers 8 s .. 8 s + 7 of tile m = k-step 2 m + s), so h_1 is split straight into qh / ql;
//   * weights: pieces 1 (q_hi) and 3 (q_lo) of every k-step of the FORWARD HALF of the split training image of the packed image
//     (diinn_pack_split_train: section WLX's piece layout on section WL's values, no division by 2 pi -- LIIF's layers 2/4/6 sit
//     in the synthesis slots), through a register ring four k-steps deep; biases from section BQ, plain;
//   * epilogue one element per k-step: relu0, split, parked in a wave-private LDS slab (a lane re-reads only what it wrote: no
//     barrier); in the last layer the three head FMAs on the unsplit activation instead, in liif_kernel's (m, g, e) order;
//   * the blend, the stores: liif_kernel's.  The Q0 rows, the head rows and bL sit in an LDS table, filled once per workgroup.
// The image's validity word is folded into bL like decode_bf16x3_kernel's: an image without it decodes to NaN.
// The body is a template on SAVE (the training forward, liif_x3_save_kernel: see the two kernels below it).
// ---------------------------------------------------------------------------------
struct LiifX3Params {
    const float* P;        // [B,H,W,1024], channels 0..255 = first-layer pre-activation of the cell (fp32 hoisted conv)
    const float* Wt;       // the LIIF packed image
    const float* split;    // its split training image (ST_FLOATS floats)
    float* out;            // [B,3,Hu,Wu]
    int B, H, W, Hu, Wu;
    LiifAxis ah, aw;
};
struct LiifX3SaveParams : LiifX3Params {    // the training forward's (a struct of its own: the inference kernel keeps its arguments)
    float* acts;           // h_1..h_4, tiled planes over the virtual pixels [4][vtiles][256][32]
    long long npix;        // N = B*Hu*Wu
};

constexpr int LIIF_X3_PREFETCH = 4;             // ring depth in k-steps (2 pieces, 3 MFMAs each)
constexpr int LIIF_X3_TAB = 7 * HID + 4;        // Q0[4][256], L[3][256], bL | validity

// issue order of a k-step (X3_KSTEP_ORDER_Q of diinn_bf16x3.hip): a weight load behind each of the first two MFMAs, the
// epilogue's VALU spread over the three
#define LIIF_X3_KSTEP_ORDER()                                                         \
    do {                                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < 3; ++i_) {                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        \
            if (i_ < 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);            \
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);                        \
        }                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                            \
    } while (0)

__device__ __forceinline__ void liif_split_bf16(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);               // exact difference: v and hi share sign and exponent range
}

template <bool SAVE, class Params>
__device__ __forceinline__ void liif_x3_body(const Params& p) {
    __shared__ __attribute__((aligned(16))) bf16x8 park[4][2][16][64];     // [wave][hi, lo][fragment][lane] = 128 KiB
    __shared__ __attribute__((aligned(16))) float tab[LIIF_X3_TAB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const float* __restrict__ Wt = p.Wt;
    {   // the tables every pixel and member share: rows 0..3 = Q0 (rel_h, rel_w, cell_h, cell_w columns), rows 4..6 = L
        if (wave < 2) {
            *(f32x4*)(tab + (2 * wave + 0) * HID + 4 * lane) = *(const f32x4*)(Wt + OFF_Q0 + (2 * wave + 0) * HID + 4 * lane);
            *(f32x4*)(tab + (2 * wave + 1) * HID + 4 * lane) = *(const f32x4*)(Wt + OFF_Q0 + (2 * wave + 1) * HID + 4 * lane);
        } else if (wave == 2) {
            *(f32x4*)(tab + 4 * HID + 4 * lane) = *(const f32x4*)(Wt + OFF_L + 0 * HID + 4 * lane);
            *(f32x4*)(tab + 5 * HID + 4 * lane) = *(const f32x4*)(Wt + OFF_L + 1 * HID + 4 * lane);
        } else {
            *(f32x4*)(tab + 6 * HID + 4 * lane) = *(const f32x4*)(Wt + OFF_L + 2 * HID + 4 * lane);
            if (lane == 0) *(f32x4*)(tab + 7 * HID) = or_bits(*(const f32x4*)(Wt + OFF_BL), SAVE ? 0u : derived_nan_mask(Wt));   // (a gathered training image carries no validity word)
        }
    }
    int x, y, b;
    [[maybe_unused]] const long long ptile = (long long)blockIdx.x * 4 + wave;   // SAVE: this wave's 32 consecutive flattened pixels
    if constexpr (SAVE) {                                       // liif_kernel<SAVE>'s ownership
        const long long pix = ptile * PLANE_TILE + j;
        const long long pc = pix < p.npix ? pix : p.npix - 1;    // lanes past the end compute on the last pixel
        const int hw = p.Hu * p.Wu;
        b = (int)(pc / hw);
        const int rem = (int)(pc - (long long)b * hw);
        y = rem / p.Wu;
        x = pix < p.npix ? rem - y * p.Wu : p.Wu;                // ... and are marked invalid below
    } else {
        x = blockIdx.x * (TILE_W * WG_TILES_X) + (wave & 1) * TILE_W + (j & (TILE_W - 1));
        y = blockIdx.y * (TILE_H * WG_TILES_Y) + (wave >> 1) * TILE_H + (j / TILE_W);
        b = blockIdx.z;
    }
    const bool valid = (x < p.Wu) && (y < p.Hu);
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane((int)(__ballot(valid) == 0ull))) return;
    const int xc = x < p.Wu ? x : p.Wu - 1;
    const int yc = y < p.Hu ? y : p.Hu - 1;

    int iy[2], ix[2];
    float rh[2], rw[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        liif_axis_eval(p.ah, yc, v, iy[v], rh[v]);
        liif_axis_eval(p.aw, xc, v, ix[v], rw[v]);
    }
    // areas in the reference's member order (vx outer, vy inner), liif.py:117-118
    float area[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) area[v] = __builtin_fabsf(rh[v >> 1] * rw[v & 1]) + 1e-9f;
    const float tot = ((area[0] + area[1]) + area[2]) + area[3];

    constexpr int PF = LIIF_X3_PREFETCH;
    static_assert(16 % PF == 0, "ring index must be static");
    constexpr int KS_BYTES = (int)(WLX_KSTEP * sizeof(float));
    constexpr int LAYER_BYTES = (int)(WLX_LAYER * sizeof(float));
    // (the ring's four k-steps past the forward half's end land in the backward half: inside the descriptor, never used)
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.split + ST_OFF_FWD), 0, (int)(ST_FLOATS * sizeof(float)), 0x00020000);
    const int lane_off = lane * 16;
    auto ld_kstep_q = [&](f32x4& qhi, f32x4& qlo, const int soff) {   // the two synthesis pieces of a k-step
        qhi = ld_piece(wrs, lane_off + 1 * PIECE_BYTES, soff);
        qlo = ld_piece(wrs, lane_off + 3 * PIECE_BYTES, soff);
    };
    bf16x8 (*mine)[16][64] = park[wave];
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;

#pragma unroll 1
    for (int v = 0; v < 4; ++v) {
        const int vh = v >> 1, vw = v & 1;
        const float relh = rh[vh], relw = rw[vw];
        const float* __restrict__ Pc = p.P + (((size_t)b * p.H + iy[vh]) * p.W + ix[vw]) * PCH + 4 * h;
        // SAVE: the two plane tiles that hold this wave's pixels of member v and the lane's place in them, as liif_kernel<SAVE>
        // derives them per member (lanes past the end carry an offset outside the descriptor's range: the store is dropped)
        [[maybe_unused]] const float* act0 = nullptr;
        [[maybe_unused]] size_t act_group = 0;
        [[maybe_unused]] int act_bytes = 0;
        [[maybe_unused]] unsigned act_voff = 0xFFFFFFF0u;
        if constexpr (SAVE) {
            const long long vtiles = (4 * p.npix + PLANE_TILE - 1) / PLANE_TILE;
            const long long vp0 = (long long)v * p.npix + ptile * PLANE_TILE;
            const long long t0 = vp0 >> 5;
            const unsigned qpos = (unsigned)(vp0 & 31) + (unsigned)j;
            act_group = (size_t)vtiles * HID * PLANE_TILE;
            act0 = p.acts + (size_t)t0 * HID * PLANE_TILE;
            act_bytes = (int)((vtiles - t0 < 2 ? vtiles - t0 : 2) * HID * (long long)PLANE_ROW_BYTES);
            if (valid) act_voff = (qpos >> 5) * (unsigned)(HID * PLANE_ROW_BYTES) + 4u * (qpos & 31) + 4u * h * PLANE_ROW_BYTES;
        }
        [[maybe_unused]] auto act_rsrc = [&](int layer) {
            return __builtin_amdgcn_make_buffer_rsrc((void*)(act0 + (size_t)layer * act_group), 0, act_bytes, 0x00020000);
        };
        f32x4 rqh[PF], rql[PF];
#pragma unroll
        for (int d = 0; d < PF; ++d) ld_kstep_q(rqh[d], rql[d], d * KS_BYTES);
        // ---- layer 1 (fp32): relu(P[cell] + W1[:, 576:580] . (rel_h, rel_w, cell_h, cell_w)), split into hi/lo fragments:
        // register r = 4g+e of tile m -> q[2m + (r>>3)][r&7]
        bf16x8 qh[16], ql[16];
        {
            const float* __restrict__ Q0 = tab + 4 * h;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c0 = 32 * m + 8 * g;
                    const f32x4 pv = *(const f32x4*)(Pc + c0);
                    const f32x4 wh = *(const f32x4*)(Q0 + 0 * HID + c0);
                    const f32x4 ww = *(const f32x4*)(Q0 + 1 * HID + c0);
                    const f32x4 wch = *(const f32x4*)(Q0 + 2 * HID + c0);
                    const f32x4 wcw = *(const f32x4*)(Q0 + 3 * HID + c0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float a = __builtin_fmaf(wh[e], relh, pv[e]);
                        a = __builtin_fmaf(ww[e], relw, a);
                        a = __builtin_fmaf(wch[e], p.ah.rel_cell, a);
                        a = __builtin_fmaf(wcw[e], p.aw.rel_cell, a);
                        a = relu0(a);
                        if constexpr (SAVE) st_act(act_rsrc(0), act_voff, (unsigned)(c0 + e) * PLANE_ROW_BYTES, a);   // h_1, unsplit
                        __bf16 sh, sl;
                        liif_split_bf16(a, sh, sl);
                        qh[2 * m + (g >> 1)][4 * (g & 1) + e] = sh;
                        ql[2 * m + (g >> 1)][4 * (g & 1) + e] = sl;
                    }
                }
            }
        }
        f32x4 sq[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) sq[g] = *(const f32x4*)(Wt + OFF_BQ + 4 * h + 8 * g);
        float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;

        // ---- layers 2..4: three copies of the layer body (a generic lambda: the member loop is not unrolled, and `#pragma unroll`
        // on a loop of this size inside it is declined); LAST is a compile-time constant per copy and fuses the head
        auto do_layer = [&](auto layer_tag) {
            constexpr int layer = decltype(layer_tag)::value;
            constexpr bool LAST = layer == 2;
            constexpr int nl = layer < 2 ? layer + 1 : 2;
            constexpr int wp = layer * LAYER_BYTES;
            const float* __restrict__ Bq = Wt + OFF_BQ + layer * HID + 4 * h;
            const float* __restrict__ Bn = Wt + OFF_BQ + nl * HID + 4 * h;
            const float* __restrict__ L = tab + 4 * HID + 4 * h;
            f32x16 ps;
            bf16x8 fh, fl;
            f32x4 l0[4], l1[4], l2[4];
            [[maybe_unused]] const __amdgpu_buffer_rsrc_t arl = act_rsrc(SAVE ? layer + 1 : 0);   // SAVE: plane h_{layer + 2}
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                f32x16 as;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) as[4 * g + e] = sq[g][e];
                if (LAST && m > 0) {                              // head rows of the tile being finished
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        l0[g] = *(const f32x4*)(L + 0 * HID + 32 * (m - 1) + 8 * g);
                        l1[g] = *(const f32x4*)(L + 1 * HID + 32 * (m - 1) + 8 * g);
                        l2[g] = *(const f32x4*)(L + 2 * HID + 32 * (m - 1) + 8 * g);
                    }
                }
#pragma unroll
                for (int ks = 0; ks < 16; ++ks) {
                    const int s = m * 16 + ks;
                    const bf16x8 wqh = __builtin_bit_cast(bf16x8, rqh[s % PF]);
                    // the two small products first, the leading one last (the order sheets.split_matmul adds them in)
                    as = MFMA_BF16(__builtin_bit_cast(bf16x8, rql[s % PF]), qh[ks], as);
                    as = MFMA_BF16(wqh, ql[ks], as);
                    as = MFMA_BF16(wqh, qh[ks], as);
                    ld_kstep_q(rqh[s % PF], rql[s % PF], wp + (s + PF) * KS_BYTES);
                    if (ks == 2) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) sq[g] = *(const f32x4*)((m < 7 ? Bq + 32 * (m + 1) : Bn) + 8 * g);
                    }
                    if (m > 0) {                                  // one epilogue element of tile m-1 per k-step
                        float a = relu0(ps[ks]);
                        asm volatile("" : "+v"(a));               // the element stays behind its k-step (see decode_bf16x3_kernel)
                        // register r of tile m-1 = channel 32(m-1) + (r&3) + 8(r>>2) + 4h: the unsplit value, as liif_kernel<SAVE> stores it
                        if constexpr (SAVE) st_act(arl, act_voff, (unsigned)(32 * (m - 1) + (ks & 3) + 8 * (ks >> 2)) * PLANE_ROW_BYTES, a);
                        if (LAST) {
                            m0 = __builtin_fmaf(l0[ks >> 2][ks & 3], a, m0);
                            m1 = __builtin_fmaf(l1[ks >> 2][ks & 3], a, m1);
                            m2 = __builtin_fmaf(l2[ks >> 2][ks & 3], a, m2);
                        } else {
                            __bf16 sh, sl;
                            liif_split_bf16(a, sh, sl);
                            fh[ks & 7] = sh;
                            fl[ks & 7] = sl;
                            if ((ks & 7) == 7) {
                                mine[0][2 * (m - 1) + (ks >> 3)][lane] = fh;
                                mine[1][2 * (m - 1) + (ks >> 3)][lane] = fl;
                            }
                        }
                    }
                    LIIF_X3_KSTEP_ORDER();
                }
                ps = as;
            }
            if (LAST) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    l0[g] = *(const f32x4*)(L + 0 * HID + 32 * 7 + 8 * g);
                    l1[g] = *(const f32x4*)(L + 1 * HID + 32 * 7 + 8 * g);
                    l2[g] = *(const f32x4*)(L + 2 * HID + 32 * 7 + 8 * g);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = relu0(ps[r]);
                if constexpr (SAVE) st_act(arl, act_voff, (unsigned)(32 * 7 + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES, a);
                if (LAST) {
                    m0 = __builtin_fmaf(l0[r >> 2][r & 3], a, m0);
                    m1 = __builtin_fmaf(l1[r >> 2][r & 3], a, m1);
                    m2 = __builtin_fmaf(l2[r >> 2][r & 3], a, m2);
                } else {
                    __bf16 sh, sl;
                    liif_split_bf16(a, sh, sl);
                    fh[r & 7] = sh;
                    fl[r & 7] = sl;
                    if ((r & 7) == 7) {
                        mine[0][14 + (r >> 3)][lane] = fh;
                        mine[1][14 + (r >> 3)][lane] = fl;
                    }
                }
            }
            if (!LAST) {                                          // the parked activation becomes the next layer's B operand
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    qh[i] = mine[0][i][lane];
                    ql[i] = mine[1][i][lane];
                }
            }
        };
        do_layer(IC<0>{});
        do_layer(IC<1>{});
        do_layer(IC<2>{});

        // ---- the ensemble weight: member v is weighted by the area of the opposite member
        m0 += __shfl_xor(m0, 32);
        m1 += __shfl_xor(m1, 32);
        m2 += __shfl_xor(m2, 32);
        float aw = area[0];                                      // area[3 - v] without dynamic register indexing
        aw = v == 0 ? area[3] : aw;
        aw = v == 1 ? area[2] : aw;
        aw = v == 2 ? area[1] : aw;
        const float wgt = aw / tot;
        o0 = __builtin_fmaf(m0 + tab[7 * HID + 0], wgt, o0);
        o1 = __builtin_fmaf(m1 + tab[7 * HID + 1], wgt, o1);
        o2 = __builtin_fmaf(m2 + tab[7 * HID + 2], wgt, o2);
    }
    if (valid && h == 0) {
        const size_t plane = (size_t)p.Hu * p.Wu;
        float* o = p.out + (size_t)b * 3 * plane + (size_t)y * p.Wu + x;
        o[0] = o0;
        o[plane] = o1;
        o[2 * plane] = o2;
    }
}

// The two instantiations.  SAVE = true is the training forward of LIIF.hip_autograd_split_bf16 (diinn_liif_train_fwd_x3): the same
// network on liif_kernel<SAVE>'s pixel ownership -- a wave owns 32 consecutive pixels of the flattened (b, y, x) index, the grid is
// ceil(N / 128) workgroups -- that also writes the unsplit fp32 relu0(a) of every hidden layer and member, h_1..h_4, to p.acts
// [4 layers][ceil(4 N / 32)][256][32] over the virtual pixels vp = v * N + pix, in liif_kernel<SAVE>'s layout and its
// two-neighbouring-tiles addressing: the planes diinn_liif_backward_data[_x3] read.  A pixel's arithmetic does not depend on the
// lane that owns it, so the output is liif_x3_kernel's bit for bit.  Every SAVE branch of the body is `if constexpr` around code
// the inference instantiation keeps whole.  (Two kernel names over one body, not one templated name: the inference kernel keeps
// its symbol.)
__global__ __launch_bounds__(256, 1) void liif_x3_kernel(const LiifX3Params p) {
    liif_x3_body<false, LiifX3Params>(p);
}

__global__ __launch_bounds__(256, 1) void liif_x3_save_kernel(const LiifX3SaveParams p) {
    liif_x3_body<true, LiifX3SaveParams>(p);
}

extern "C" {

// diinn_liif_decode's checks in its order, with split_dev among the pointers
int diinn_liif_decode_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* split_dev,
                         float* workspace_dev, float* out_dev, int B, int H, int W, int Hu, int Wu) {
    if (!all_set(feat_dev, packed_dev, split_dev, out_dev, workspace_dev)) return DIINN_ERR_INVALID_ARG;
    if (int st = check_dims(B, H, W)) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if (int st = check_extent(Hu, Wu)) return st;
    int gx, gy, gz, blk;
    diinn_decode_launch_info(B, Hu, Wu, 0, Hu, &gx, &gy, &gz, &blk);
    if (int st = check_grid(gy, gz)) return st;                  // every argument is judged before the first launch
    if (int st = launch_P(stream, feat_dev, packed_dev, workspace_dev, B, H, W, 0, H, 4)) return st;   // diinn_liif_decode's P
    LiifX3Params p;
    p.P = workspace_dev; p.Wt = packed_dev; p.split = split_dev; p.out = out_dev;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu;
    p.ah = make_liif_axis(H, Hu);
    p.aw = make_liif_axis(W, Wu);
    hipLaunchKernelGGL(liif_x3_kernel, dim3(gx, gy, gz), dim3(blk), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

// diinn_liif_decode_x3's checks in its order, with acts_dev among the pointers and diinn_liif_train_fwd's limits (the virtual
// pixels, the 1-D grid) in the place of the inference grid's
int diinn_liif_train_fwd_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* split_dev,
                            float* workspace_dev, float* out_dev, float* acts_dev, int B, int H, int W, int Hu, int Wu) {
    if (!all_set(feat_dev, packed_dev, split_dev, out_dev, workspace_dev, acts_dev)) return DIINN_ERR_INVALID_ARG;
    if (int st = check_dims(B, H, W)) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if (int st = check_extent(Hu, Wu)) return st;
    const long long npix = (long long)B * Hu * Wu;
    if (int st = check_npix(4 * npix)) return st;                // the limit applies to the virtual pixels
    const long long blocks = ((npix + PLANE_TILE - 1) / PLANE_TILE + 3) / 4;
    if (blocks > 2147483000LL) return DIINN_ERR_TOO_LARGE;       // every argument is judged before the first launch
    if (int st = launch_P(stream, feat_dev, packed_dev, workspace_dev, B, H, W, 0, H, 4)) return st;   // diinn_liif_decode's P
    LiifX3SaveParams p;
    p.P = workspace_dev; p.Wt = packed_dev; p.split = split_dev; p.out = out_dev;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu;
    p.ah = make_liif_axis(H, Hu);
    p.aw = make_liif_axis(W, Wu);
    p.acts = acts_dev; p.npix = npix;
    hipLaunchKernelGGL(liif_x3_save_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

}  // extern "C"
