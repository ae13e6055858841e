// diinn_liif_training.hip -- the LIIF comparison decoder under autograd: the per-virtual-pixel backward chain and the per-cell sum
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h)
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// Backward pass of liif_kernel (training; reference: autograd through LIIF.query_rgb, liif.py:59-127).
// Per HR pixel p and ensemble member v = 2 vh + vw (the VIRTUAL pixel vp = v * N + p, N = B Hu Wu):
//     a_1 = P1[c_v] + Wc r_v,  h_1 = relu(a_1),  a_l = W_l h_{l-1} + b_l,  h_l = relu(a_l)  (l = 2..4),  pred_v = L h_4 + bL,
//     out = sum_v w_v pred_v,  w_v = area[3 - v] / tot.
// With g = d loss / d out and the planes h_1..h_4 saved by liif_kernel<SAVE> (a post-ReLU value is its own mask):
//     g_a,4 = (L^T (w_v g)) [h_4 > 0],     g_a,l-1 = (W_l^T g_a,l) [h_{l-1} > 0]     (a zero or a NaN closes the gate).
// liif_bwd_layer_kernel : bwd_layer_kernel<HEAD, KPART=false>'s scheme with a ReLU gate.  One launch per layer l = 4, 3, 2 (li = l - 1
//                    = 3, 2, 1 counts the planes from 0).  A wave owns one plane tile of 32 virtual pixels, holds their 256 values of
//                    g_a,l in registers as the MFMA B operand (rows read in accumulator order: no shuffle), streams the transposed
//                    weight W_l^T -- the synthesis pieces (part 1) of section WLT, where pack_liif puts imnet.layers.{2,4,6} -- exactly
//                    as liif_kernel streams WL, and its epilogue gates with h_{l-1} > 0 and writes g_a,l-1.
//                    HEAD (l = 4): the wave computes its own operand from the plain gout planes, the head L and the member's area
//                    weight -- recomputed with liif_kernel's expressions in its order, so it is the forward's weight bit for bit --
//                    gates it with the saved h_4 and stores it (g_a,4 is the A operand of dW_4).
// liif_cell_sum_kernel  : dP1[b, ch, cy, cx] = sum over the members v and the pixels p with c_v(p) = (cy, cx) of g_a,1.  Each member's
//                    index table is monotone (liif_axis_eval is a composition of monotone fp32 steps), so per member a cell's pixels
//                    are a rectangle [seg_h[vh][cy], seg_h[vh][cy+1]) x [seg_w[vw][cx], seg_w[vw][cx+1]): four rectangles per cell,
//                    added in member order, rows top to bottom, left to right inside a row.  No atomics.
// Every plane group here is [ceil(4 N / 32)][256][32] over the virtual pixels: acts [4] (h_1..h_4), G [4] (g_a,1..g_a,4).
// The parameter gradients are GEMMs over that axis on diinn_plane_gemm_nt / diinn_plane_rowdot (liif_training.py).
// ---------------------------------------------------------------------------------
struct LiifBwdParams {
    const float* Wt;         // packed image (sections WLT, L)
    const float* acts;       // h_1..h_4
    const float* gout;       // [3][N] plain planes: d loss / d out
    float* G;                // g_a,1..g_a,4
    long long npix;          // N = B*Hu*Wu
    long long vpix, ntiles;  // 4 N and its tiles
    int layer;               // li: consumes G[li], produces G[li-1]
    int Hu, Wu;
    LiifAxis ah, aw;
};

__device__ __forceinline__ float ld_plane_nt(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 2));
}

template <bool HEAD>
__global__ __launch_bounds__(256, 1) void liif_bwd_layer_kernel(const LiifBwdParams p) {
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

    // HEAD: w_v g of this lane's virtual pixel (liif_kernel's area weight, term for term)
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

    // B operand: register kk = 16m + r of lane-half h holds channel chan_of(kk, h) of this lane's virtual pixel.  The first BLD
    // k-groups are fetched up front, the rest stream in BLD groups ahead of the MFMAs of the first output tile.
    constexpr int BLD = 8;
    float gs[128];
    auto load_group = [&](int kg) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kk = 4 * kg + e;
            const unsigned so = (unsigned)(32 * (kk >> 4) + (kk & 3) + 8 * ((kk & 15) >> 2)) * PLANE_ROW_BYTES;
            gs[kk] = ld_plane_nt(HEAD ? act_li : inG, voff, so);   // HEAD: h_4, turned into g_a,4 by head_group
        }
    };
    auto head_group = [&](int kg) {
        const float* __restrict__ L = p.Wt + OFF_L;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kk = 4 * kg + e;
            const int c0 = 32 * (kk >> 4) + (kk & 3) + 8 * ((kk & 15) >> 2);      // channel of lane-half 0; half 1: + 4
            const float l0 = h ? L[c0 + 4] : L[c0], l1 = h ? L[HID + c0 + 4] : L[HID + c0], l2 = h ? L[2 * HID + c0 + 4] : L[2 * HID + c0];
            float g = l0 * wg0;
            g = __builtin_fmaf(l1, wg1, g);
            g = __builtin_fmaf(l2, wg2, g);
            gs[kk] = gs[kk] > 0.0f ? g : 0.0f;
        }
    };
    auto head_store_group = [&](int kg) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kk = 4 * kg + e;
            const unsigned so = (unsigned)(32 * (kk >> 4) + (kk & 3) + 8 * ((kk & 15) >> 2)) * PLANE_ROW_BYTES;
            st_act(inG, voff, so, gs[kk]);
        }
    };
#pragma unroll
    for (int kg = 0; kg < BLD; ++kg) load_group(kg);

    constexpr int PF = DECODE_PREFETCH;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.Wt, 0, (int)(PACKED_FLOATS * sizeof(float)), 0x00020000);   // reads past the end return 0
    const int lane_off = lane * 16;
    const int wp = (int)((OFF_WLT + (size_t)(li - 1) * WL_LAYER) * sizeof(float));
    f32x4 rq[PF];
#pragma unroll
    for (int d = 0; d < PF; ++d) rq[d] = ld_piece(wrs, lane_off, wp + (2 * d + 1) * PIECE_BYTES);

    f32x16 pg;                                                   // finished tile of W_l^T g_a,l
    float kt[16];                                                // saved h_{l-1} of the tile being finished
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        f32x16 as;
#pragma unroll
        for (int r = 0; r < 16; ++r) as[r] = 0.0f;
#pragma unroll
        for (int kg = 0; kg < WL_KG; ++kg) {
            const int s = m * WL_KG + kg;
            const f32x4 wq = rq[s % PF];
            if constexpr (HEAD) {
                if (m == 0) head_group(kg);                       // (its loads went out BLD groups = 32 MFMAs ago)
                if (m == 1) head_store_group(kg);                 // 4 stores behind 4 MFMAs
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) as = MFMA32(wq[e], gs[4 * kg + e], as);
            rq[s % PF] = ld_piece(wrs, lane_off, wp + (2 * (s + PF) + 1) * PIECE_BYTES);
            if (m == 0 && kg + BLD < WL_KG) load_group(kg + BLD); // rest of the B operand, BLD groups ahead
            if (m > 0 && kg == 0) {                               // saved plane of tile m-1, used from kg = 8 on
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    kt[r] = ld_plane_nt(act, voff, (unsigned)(32 * (m - 1) + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES);
            }
            if (m > 0 && kg >= 8 && kg < 24) {                    // one epilogue element of tile m-1 every 4 MFMAs
                const int r = kg - 8;
                st_act(outG, voff, (unsigned)(32 * (m - 1) + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES, kt[r] > 0.0f ? pg[r] : 0.0f);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) pg[r] = as[r];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) kt[r] = ld_plane_nt(act, voff, (unsigned)(32 * 7 + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        st_act(outG, voff, (unsigned)(32 * 7 + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES, kt[r] > 0.0f ? pg[r] : 0.0f);
}

// ---------------------------------------------------------------------------------
// liif_cell_sum_kernel: one thread per (cell, channel), the cells of an image flattened over the threads (cx fastest: neighbouring
// lanes read neighbouring column segments of the same HR rows).  Output in both of cell_sum_kernel's layouts -- NCHW planes 0..255
// of a [B][1024][H][W] buffer and rows 0..255 of a tiled group [ceil(B H W / 32)][1024][32] over the CELL axis -- so that the hoisted
// conv's gradients run unchanged on them with rows = 256.  A cell that owns no virtual pixel gets zeros; rows >= 256 and the
// padding of a ragged last tile are not written.  HBM-bound (reads g_a,1 once).
// ---------------------------------------------------------------------------------
struct LiifCellSumParams {
    const float* G1;         // tiled [vtiles][256][32]: g_a,1 over the virtual pixels
    float* dP;               // [B][1024][H][W], planes 0..255 written
    float* dP_tiled;         // [ceil(B*H*W / 32)][1024][32], rows 0..255 written
    const int* seg_h;        // [2][H+1]: first HR row of every LR row for vh = 0, 1 (last entry Hu)
    const int* seg_w;        // [2][W+1]
    int B, H, W, Hu, Wu;
    long long npix;          // N
};

__global__ __launch_bounds__(256) void liif_cell_sum_kernel(const LiifCellSumParams p) {
    const int cell = blockIdx.x * 256 + threadIdx.x;                 // cy * W + cx
    if (cell >= p.H * p.W) return;
    const int b = blockIdx.y;
    const int cy = cell / p.W, cx = cell - cy * p.W;
    const int ch = blockIdx.z;
    const float* __restrict__ src = p.G1 + (size_t)ch * PLANE_TILE;
    auto at = [&](long long vp) { return src + (size_t)(vp >> 5) * (HID * PLANE_TILE) + (size_t)(vp & 31); };
    float acc = 0.0f;
#pragma unroll 1
    for (int v = 0; v < 4; ++v) {
        const int* __restrict__ sh = p.seg_h + (v >> 1) * (p.H + 1);
        const int* __restrict__ sw = p.seg_w + (v & 1) * (p.W + 1);
        // (clamped: a bad table must not steer a load outside G1)
        const int y0 = max(sh[cy], 0), y1 = min(sh[cy + 1], p.Hu);
        const int x0 = max(sw[cx], 0), x1 = min(sw[cx + 1], p.Wu);
        float mv = 0.0f;
        for (int y = y0; y < y1; ++y) {
            const long long row = (long long)v * p.npix + ((long long)b * p.Hu + y) * p.Wu;
            float r = 0.0f;
            for (int x = x0; x < x1; ++x) r += __builtin_nontemporal_load(at(row + x));
            mv += r;
        }
        acc += mv;
    }
    p.dP[(((size_t)b * PCH + ch) * p.H + cy) * p.W + cx] = acc;
    const long long n = (long long)b * p.H * p.W + cell;
    p.dP_tiled[((size_t)(n >> 5) * PCH + ch) * PLANE_TILE + (size_t)(n & 31)] = acc;
}

extern "C" {

int diinn_liif_backward_data(void* stream, const float* gout_planes_dev, const float* acts_dev, const float* packed_dev,
                             float* G_dev, int B, int H, int W, int Hu, int Wu) {
    if (!gout_planes_dev || !acts_dev || !packed_dev || !G_dev) return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if ((double)Hu * Wu >= 2.0e9) return DIINN_ERR_TOO_LARGE;
    const long long npix = (long long)B * Hu * Wu;
    st = check_npix(4 * npix);                                   // the limit applies to the virtual pixels
    if (st) return st;
    if (((size_t)packed_dev) & 15) return DIINN_ERR_INVALID_ARG; // 16-byte weight pieces
    LiifBwdParams p;
    p.Wt = packed_dev; p.acts = acts_dev; p.gout = gout_planes_dev; p.G = G_dev;
    p.npix = npix; p.vpix = 4 * npix; p.ntiles = (p.vpix + PLANE_TILE - 1) / PLANE_TILE;
    p.Hu = Hu; p.Wu = Wu;
    p.ah = make_liif_axis(H, Hu);
    p.aw = make_liif_axis(W, Wu);
    if ((p.ntiles + 3) / 4 > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    const unsigned blocks = (unsigned)((p.ntiles + 3) / 4);
    for (int layer = 3; layer >= 1; --layer) {
        p.layer = layer;
        if (layer == 3) hipLaunchKernelGGL(liif_bwd_layer_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(liif_bwd_layer_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_status(e);
    }
    return DIINN_OK;
}

int diinn_liif_cell_sum(void* stream, const float* G1_dev, const int32_t* seg_h_dev, const int32_t* seg_w_dev,
                        float* dP_dev, float* dP_tiled_dev, int B, int H, int W, int Hu, int Wu) {
    if (!G1_dev || !seg_h_dev || !seg_w_dev || !dP_dev || !dP_tiled_dev) return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if ((double)Hu * Wu >= 2.0e9) return DIINN_ERR_TOO_LARGE;
    const long long npix = (long long)B * Hu * Wu;
    st = check_npix(4 * npix);
    if (st) return st;
    if (B > 65535 || (long long)H * W > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    LiifCellSumParams p{G1_dev, dP_dev, dP_tiled_dev, seg_h_dev, seg_w_dev, B, H, W, Hu, Wu, npix};
    hipLaunchKernelGGL(liif_cell_sum_kernel, dim3((unsigned)(((long long)H * W + 255) / 256), (unsigned)B, HID), dim3(256), 0,
                       (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

}  // extern "C"
