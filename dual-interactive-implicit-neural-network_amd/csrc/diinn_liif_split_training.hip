// diinn_liif_split_training.hip -- the LIIF comparison decoder under autograd in split-bf16 arithmetic (behind
// LIIF.hip_autograd_split_bf16): the backward pass of the per-virtual-pixel chain on v_mfma_f32_32x32x16_bf16.
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h.  The forward of the same switch is
// liif_x3_save_kernel in diinn_liif_x3.hip.)
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// liif_bwd_layer_x3_kernel<HEAD>: liif_bwd_layer_kernel<HEAD> (diinn_liif_training.hip) on the bf16 matrix cores -- the Q-only half of
// bwd_layer_x3_kernel (diinn_split_training.hip).
//     g_a,l-1 = (W_l^T g_a,l) [h_{l-1} > 0]
// with the product's operands carried as hi + lo (hi = bf16(v), lo = bf16(v - hi)) and the product evaluated as
// w_lo.g_hi + w_hi.g_lo + w_hi.g_hi on ONE fp32 accumulator: the two small products first, the leading one last (the order
// sheets.split_matmul adds them in).  One launch per layer l = 4, 3, 2 (li = l - 1 = 3, 2, 1 counts the planes from 0).
//   * A wave owns one plane tile of 32 virtual pixels.  Its B operand g_a,l -- 256 values per virtual pixel -- is split ONCE per
//     tile, in registers: accumulator-order registers 8 ks .. 8 ks + 7 of the fp32 kernel's operand are the fragment of k-step ks
//     (chan_of_bf16(ks, h, j) = chan_of(8 ks + j, h)), so hi and lo are 2 x 16 fragments of 4 registers = 128 VGPRs, reused over all
//     8 output tiles.  The fp32 values are fetched four k-steps ahead of the first output tile's MFMAs and split right before the
//     k-step that needs them.
//   * HEAD (l = 4): the loads fetch the saved h_4 instead; a k-step's 8 values are turned into g_a,4 = (L^T (w_v g)) [h_4 > 0] with
//     liif_bwd_layer_kernel<true>'s expressions in its order and in fp32 -- the area weight recomputed with liif_kernel's
//     expressions, L^T (w_v g) as its FMA chain -- and stored unsplit (g_a,4 is the A operand of dW_4): on the same acts, G[3] is
//     the fp32 entry point's G[3] bit for bit.
//   * A operand: pieces 1 (q_hi) and 3 (q_lo) of every k-step of the BACKWARD HALF of the split training image (ST_OFF_BWD: the
//     hi/lo pieces of the transposed layers from section WLT, where pack_liif puts imnet.layers.{2,4,6}), layer li - 1, through a
//     register ring four k-steps deep over a buffer descriptor, as the forward streams its half.
//   * Epilogue: the fp32 kernel's -- gate with the saved h_{l-1} > 0 (a zero or a NaN closes the gate), fp32 g_a,l-1 to the same
//     plane addresses -- one element of tile m-1 per k-step of tile m; the saved plane of a tile is fetched half a tile ahead.
//     The accumulator-to-channel map of the 32 x 32 tile is the fp32 MFMA's, so the plane addressing is that kernel's.
// Every plane access goes through a descriptor over the wave's own tile; lanes past 4 N carry an offset outside it (loads return
// 0, stores are dropped).  No LDS, no scratch, one wave per SIMD.
// ---------------------------------------------------------------------------------
struct LiifBwdX3Params {
    const float* Wt;         // packed image: the head rows L (HEAD)
    const float* split;      // split training image: pieces 1 / 3 of the backward half are streamed
    const float* acts;       // h_1..h_4
    const float* gout;       // [3][N] plain planes: d loss / d out
    float* G;                // g_a,1..g_a,4
    long long npix;          // N = B*Hu*Wu
    long long vpix, ntiles;  // 4 N and its tiles
    int layer;               // li: consumes G[li] (HEAD: computes it), produces G[li-1]
    int Hu, Wu;
    LiifAxis ah, aw;
};

__device__ __forceinline__ static float ld_plane_nt(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 2));   // nt: read once
}

__device__ __forceinline__ static void split2_bf16(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);               // exact difference: v and hi share sign and exponent range
}

template <bool HEAD>
__global__ __launch_bounds__(256, 1) void liif_bwd_layer_x3_kernel(const LiifBwdX3Params p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const long long tile = (long long)blockIdx.x * 4 + wave;
    if (tile >= p.ntiles) return;                                // wave-uniform
    const long long vp = tile * PLANE_TILE + j;
    const bool valid = vp < p.vpix;

    const int li = p.layer;                                     // 1..3
    const size_t group = (size_t)p.ntiles * HID * PLANE_TILE;   // floats per layer of acts / G
    // lanes past the end: offset outside the descriptor, loads return 0 and stores are dropped
    const unsigned voff = valid ? 4u * j + 4u * h * PLANE_ROW_BYTES : 0xFFFFFFF0u;
    const __amdgpu_buffer_rsrc_t inG = tile_rsrc(p.G + (size_t)li * group, tile, HID);        // HEAD: written here
    const __amdgpu_buffer_rsrc_t act = tile_rsrc(p.acts + (size_t)(li - 1) * group, tile, HID);
    const __amdgpu_buffer_rsrc_t act_li = tile_rsrc(p.acts + (size_t)li * group, tile, HID);
    const __amdgpu_buffer_rsrc_t outG = tile_rsrc(p.G + (size_t)(li - 1) * group, tile, HID);

    // HEAD: w_v g of this lane's virtual pixel (liif_kernel's area weight, term for term: liif_bwd_layer_kernel<true>'s code)
    float wg0 = 0.0f, wg1 = 0.0f, wg2 = 0.0f;
    if constexpr (HEAD) {
        if (valid) {
            const int v = (int)(vp / p.npix);
            const long long pix = vp - (long long)v * p.npix;
            const int hw = p.Hu * p.Wu;
            const int rem = (int)(pix % hw);
            const int y = rem / p.Wu, x = rem - y * p.Wu;
            int iy, ix;
            float rh[2], rw[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                liif_axis_eval(p.ah, y, u, iy, rh[u]);
                liif_axis_eval(p.aw, x, u, ix, rw[u]);
            }
            float area[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) area[u] = __builtin_fabsf(rh[u >> 1] * rw[u & 1]) + 1e-9f;
            const float tot = ((area[0] + area[1]) + area[2]) + area[3];
            float aw = area[0];                                  // area[3 - v]
            aw = v == 0 ? area[3] : aw;
            aw = v == 1 ? area[2] : aw;
            aw = v == 2 ? area[1] : aw;
            const float wgt = aw / tot;
            wg0 = wgt * p.gout[pix];
            wg1 = wgt * p.gout[(size_t)p.npix + pix];
            wg2 = wgt * p.gout[2 * (size_t)p.npix + pix];
        }
    }

    // B operand.  Fragment element e of k-step ks = register kk = 8 ks + e of the fp32 kernel's operand = channel
    // 32 (kk >> 4) + (kk & 3) + 8 ((kk & 15) >> 2) + 4 h of this lane's virtual pixel.
    constexpr int BLD = 4;                                       // k-steps the fp32 values are fetched ahead
    bf16x8 gh[16], gl[16];
    float fa[16][8];                                             // fp32 staging: a row lives from its loads to its split
    auto row_of = [](int kk) { return (unsigned)(32 * (kk >> 4) + (kk & 3) + 8 * ((kk & 15) >> 2)); };
    auto load_step = [&](const int ks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) fa[ks][e] = ld_plane_nt(HEAD ? act_li : inG, voff, row_of(8 * ks + e) * PLANE_ROW_BYTES);   // HEAD: h_4
    };
    auto split_step = [&](const int ks) {
        const float* __restrict__ L = p.Wt + OFF_L;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = fa[ks][e];
            if constexpr (HEAD) {                                // h_4 -> g_a,4: liif_bwd_layer_kernel<true>'s head_group, term for term
                const int c0 = (int)row_of(8 * ks + e);          // channel of lane-half 0; half 1: + 4
                const float l0 = h ? L[c0 + 4] : L[c0], l1 = h ? L[HID + c0 + 4] : L[HID + c0], l2 = h ? L[2 * HID + c0 + 4] : L[2 * HID + c0];
                float g = l0 * wg0;
                g = __builtin_fmaf(l1, wg1, g);
                g = __builtin_fmaf(l2, wg2, g);
                a = a > 0.0f ? g : 0.0f;
                st_act(inG, voff, (unsigned)c0 * PLANE_ROW_BYTES, a);   // unsplit
            }
            __bf16 vh, vl;
            split2_bf16(a, vh, vl);
            gh[ks][e] = vh; gl[ks][e] = vl;
        }
    };
#pragma unroll
    for (int ks = 0; ks < BLD; ++ks) load_step(ks);

    // A operand: the two synthesis pieces of a k-step by immediate offsets from one scalar offset
    constexpr int PF = 4;
    constexpr int KS_BYTES = (int)(WLX_KSTEP * sizeof(float));
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.split, 0, (int)(ST_FLOATS * sizeof(float)), 0x00020000);
    const int lane_off = lane * 16;
    const int wp = (int)((ST_OFF_BWD + (size_t)(li - 1) * WLX_LAYER) * sizeof(float));
    f32x4 rqh[PF], rql[PF];
    auto ld_kstep_q = [&](const int d, const int soff) {
        rqh[d] = ld_piece(wrs, lane_off + 1 * PIECE_BYTES, soff);
        rql[d] = ld_piece(wrs, lane_off + 3 * PIECE_BYTES, soff);
    };
#pragma unroll
    for (int d = 0; d < PF; ++d) ld_kstep_q(d, wp + d * KS_BYTES);

    f32x16 pg;                                                   // finished tile of W_l^T g_a,l
    float kt[16], ktn[16];                                       // saved h_{l-1} of the tile being finished / of the one in flight
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        f32x16 as;
#pragma unroll
        for (int r = 0; r < 16; ++r) as[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int s = m * 16 + ks;
            if (m == 0) split_step(ks);                           // (its loads went out BLD k-steps ago)
            const bf16x8 wqh = __builtin_bit_cast(bf16x8, rqh[s % PF]);
            // the two small products first, the leading one last (the forward's order)
            as = MFMA_BF16(__builtin_bit_cast(bf16x8, rql[s % PF]), gh[ks], as);
            as = MFMA_BF16(wqh, gl[ks], as);
            as = MFMA_BF16(wqh, gh[ks], as);
            if (s + PF < 128) ld_kstep_q(s % PF, wp + (s + PF) * KS_BYTES);   // (a launch is one layer: nothing to fetch past its end,
                                                                               //  and layer 3's end is the image's end)
            if (m == 0 && ks + BLD < 16) load_step(ks + BLD);     // rest of the B operand, BLD k-steps ahead
            if (ks == 8) {                                        // saved plane of tile m, used from the next tile's first k-step on
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    ktn[r] = ld_plane_nt(act, voff, (unsigned)(32 * m + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES);
            }
            if (m > 0)                                            // one epilogue element of tile m-1 per k-step
                st_act(outG, voff, (unsigned)(32 * (m - 1) + (ks & 3) + 8 * (ks >> 2)) * PLANE_ROW_BYTES, kt[ks] > 0.0f ? pg[ks] : 0.0f);
            __builtin_amdgcn_sched_barrier(0);                    // the region ends at the k-step
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pg[r] = as[r];
            kt[r] = ktn[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
        st_act(outG, voff, (unsigned)(32 * 7 + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES, kt[r] > 0.0f ? pg[r] : 0.0f);
}

extern "C" {

// diinn_liif_backward_data's checks in its order, with split_dev among the pointers and 16-byte aligned like packed_dev
int diinn_liif_backward_data_x3(void* stream, const float* gout_planes_dev, const float* acts_dev, const float* packed_dev,
                                const float* split_dev, float* G_dev, int B, int H, int W, int Hu, int Wu) {
    if (!gout_planes_dev || !acts_dev || !packed_dev || !split_dev || !G_dev) return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if ((double)Hu * Wu >= 2.0e9) return DIINN_ERR_TOO_LARGE;
    const long long npix = (long long)B * Hu * Wu;
    st = check_npix(4 * npix);                                   // the limit applies to the virtual pixels
    if (st) return st;
    if ((((size_t)packed_dev) | ((size_t)split_dev)) & 15) return DIINN_ERR_INVALID_ARG;   // 16-byte weight pieces
    LiifBwdX3Params p;
    p.Wt = packed_dev; p.split = split_dev; p.acts = acts_dev; p.gout = gout_planes_dev; p.G = G_dev;
    p.npix = npix; p.vpix = 4 * npix; p.ntiles = (p.vpix + PLANE_TILE - 1) / PLANE_TILE;
    p.Hu = Hu; p.Wu = Wu;
    p.ah = make_liif_axis(H, Hu);
    p.aw = make_liif_axis(W, Wu);
    if ((p.ntiles + 3) / 4 > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    const unsigned blocks = (unsigned)((p.ntiles + 3) / 4);
    for (int layer = 3; layer >= 1; --layer) {
        p.layer = layer;
        if (layer == 3) hipLaunchKernelGGL(liif_bwd_layer_x3_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(liif_bwd_layer_x3_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_status(e);
    }
    return DIINN_OK;
}

}  // extern "C"
