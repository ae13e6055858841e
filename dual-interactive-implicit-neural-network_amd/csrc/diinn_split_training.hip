// diinn_split_training.hip -- mode 3 under autograd in split-bf16 arithmetic (behind ImplicitDecoder.hip_autograd_split_bf16):
// the device packer of the split training image and the backward pass of the per-pixel chain on v_mfma_f32_32x32x16_bf16.
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h.  The forward of the same switch is
// decode_bf16x3_kernel<SIN | X3_SAVE> in diinn_bf16x3.hip.)
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// split_train_pack_kernel: sections WL and WLT of a (gathered) training image -> the two halves of the split training image
// (diinn_layout.h "the SPLIT TRAINING image").  chan_of_bf16(ks, h, j) = chan_of(8 ks + j, h): a thread owns one lane of one piece
// pair -- its eight weights are two 16-byte runs of the source, (kg = 2 ks, e 0..3) and (kg = 2 ks + 1, e 0..3) of the same lane --
// and writes them as one 16-byte hi and one 16-byte lo run.  hi = bf16(w), lo = bf16(w - hi), round to nearest even, as the host
// packer (diinn_pack_split_train_host is the twin; the tests compare the two bit for bit).  3 MiB written: runs once per weight version.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ static void split2_bf16(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);               // exact difference: v and hi share sign and exponent range
}

constexpr int ST_PACK_THREADS = 2 * 3 * 8 * 16 * 2 * 64;        // [half][layer][m][ks][part][lane] = 98,304

__global__ __launch_bounds__(256) void split_train_pack_kernel(const float* __restrict__ image, float* __restrict__ split) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ST_PACK_THREADS) return;
    const int lane = t & 63, part = (t >> 6) & 1, ks = (t >> 7) & 15, m = (t >> 11) & 7;
    const int hl = t >> 14, half = hl / 3, layer = hl - 3 * half;
    const float* __restrict__ src = image + (half ? OFF_WLT : OFF_WL) + (size_t)layer * WL_LAYER +
                                    (((size_t)m * WL_KG + 2 * ks) * 2 + part) * WL_PIECE + lane * 4;
    const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 2 * WL_PIECE);
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        __bf16 vh, vl;
        split2_bf16(a[e], vh, vl);
        hi[e] = vh; lo[e] = vl;
        split2_bf16(b[e], vh, vl);
        hi[4 + e] = vh; lo[4 + e] = vl;
    }
    bf16x8* __restrict__ dst = (bf16x8*)(split + (half ? ST_OFF_BWD : ST_OFF_FWD)) +
                               ((((size_t)layer * 8 + m) * 16 + ks) * 4 + part) * 64 + lane;
    dst[0] = hi;
    dst[2 * 64] = lo;
}

// ---------------------------------------------------------------------------------
// bwd_layer_x3_kernel<HEAD>: bwd_layer_kernel<HEAD, KPART = true> (diinn_training.hip) on the bf16 matrix cores.
//     g_q,i-1 = Wq_i^T g_a,i + Qw_i^T g_s,i
// with every operand carried as hi + lo (hi = bf16(v), lo = bf16(v - hi)) and a product evaluated as lo.hi + hi.lo + hi.hi with fp32
// accumulation, the forward's rule and order (decode_bf16x3_kernel: the two small products first, the leading one last).
//   * A wave owns one plane tile (32 pixels).  Its B operand (g_a,i ; g_s,i) -- 512 values per pixel -- is split ONCE per tile, in
//     registers: accumulator-order registers 8 ks .. 8 ks + 7 of the fp32 kernel's operand are the fragment of k-step ks
//     (chan_of_bf16(ks, h, j) = chan_of(8 ks + j, h)), so hi/lo of both halves are 4 x 16 fragments of 4 registers = 256 VGPRs, the
//     fp32 operand's count, reused over all 8 output tiles.  The fp32 values are fetched four k-steps ahead of the first output
//     tile's MFMAs and split right before the k-step that needs them.
//   * HEAD (layer 3): the loads fetch (k_3, s_3) instead, a k-step's 16 values are turned into (g_a,3 ; g_s,3) with
//     g_q,3 = L^T g_out -- bwd_head_kernel's arithmetic term for term -- and G_3, q_3 are stored from there (fp32, unsplit).
//   * A operand: the backward half of the split training image, [layer][m][ks][k_hi, q_hi, k_lo, q_lo][lane][j] -- the hi/lo pieces
//     of Wq_i^T (against g_a) and Qw_i^T (against g_s) -- through a register ring four k-steps deep, as the forward streams WLX.
//   * Epilogue: gate_store as in the fp32 kernel -- dsincos, the gates of layer i-1, G_{i-1} and q_{i-1} to the same fp32 planes
//     -- one element of tile m-1 per k-step of tile m; the saved k, s of a tile are fetched half a tile ahead.  The
//     accumulator-to-channel map of the 32 x 32 tile is the fp32 MFMA's, so the plane addressing is that kernel's.
// Mode 3 only (no KPART = false, no 3x3 head, no init_q).  No LDS, no scratch, one wave per SIMD.
// ---------------------------------------------------------------------------------
struct BwdX3Params {
    const float* Wt;         // (gathered) training image: the head rows L (HEAD)
    const float* split;      // split training image: the backward half is streamed
    const float* acts;       // k_i (rows 0..255), s_i (rows 256..511)
    const float* gout;       // [3][npix] plain planes: d loss / d out
    float* G;                // g_a,i (rows 0..255), g_s,i (rows 256..511)
    float* Q;                // q_i
    long long npix, ntiles;
    int layer;               // consumes G_layer (HEAD: computes it), produces G_{layer-1}, Q_{layer-1}
};

__device__ __forceinline__ static float ld_plane_nt(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 2));   // nt: read once
}

template <bool HEAD>
__global__ __launch_bounds__(256, 1) void bwd_layer_x3_kernel(const BwdX3Params p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const long long tile = (long long)blockIdx.x * 4 + wave;
    if (tile >= p.ntiles) return;                                // wave-uniform
    const bool valid = tile * PLANE_TILE + j < p.npix;

    const int li = p.layer;                                     // 1..3
    const size_t agroup = (size_t)p.ntiles * ACT_ROWS * PLANE_TILE;     // floats per layer of acts / G
    const size_t qgroup = (size_t)p.ntiles * HID * PLANE_TILE;
    // lanes past the end: offset outside the descriptor, loads return 0 and stores are dropped
    const unsigned voff = valid ? 4u * j + 4u * h * PLANE_ROW_BYTES : 0xFFFFFFF0u;
    // the operand's source: G_li, or with HEAD the saved planes of layer li
    const __amdgpu_buffer_rsrc_t src = tile_rsrc((HEAD ? p.acts : p.G) + (size_t)li * agroup, tile, ACT_ROWS);
    const __amdgpu_buffer_rsrc_t act = tile_rsrc(p.acts + (size_t)(li - 1) * agroup, tile, ACT_ROWS);
    const __amdgpu_buffer_rsrc_t outG = tile_rsrc(p.G + (size_t)(li - 1) * agroup, tile, ACT_ROWS);
    const __amdgpu_buffer_rsrc_t outQ = tile_rsrc(p.Q + (size_t)(li - 1) * qgroup, tile, HID);
    const __amdgpu_buffer_rsrc_t outG_li = tile_rsrc(p.G + (size_t)li * agroup, tile, ACT_ROWS);     // HEAD
    const __amdgpu_buffer_rsrc_t outQ_li = tile_rsrc(p.Q + (size_t)li * qgroup, tile, HID);          // HEAD

    float go0 = 0.0f, go1 = 0.0f, go2 = 0.0f;                    // HEAD: d loss / d out of this lane's pixel
    if constexpr (HEAD) {
        const long long pix = tile * PLANE_TILE + j;
        if (valid) {
            go0 = p.gout[pix];
            go1 = p.gout[(size_t)p.npix + pix];
            go2 = p.gout[2 * (size_t)p.npix + pix];
        }
    }

    // B operand.  Fragment element j of k-step ks = register kk = 8 ks + j of the fp32 kernel's operand = channel
    // 32 (kk >> 4) + (kk & 3) + 8 ((kk & 15) >> 2) + 4 h of this lane's pixel.
    constexpr int BLD = 4;                                       // k-steps the fp32 values are fetched ahead
    bf16x8 gah[16], gal[16], gsh[16], gsl[16];
    float fa[16][8], fs[16][8];                                  // fp32 staging: a row lives from its loads to its split
    auto row_of = [](int kk) { return (unsigned)(32 * (kk >> 4) + (kk & 3) + 8 * ((kk & 15) >> 2)); };
    auto load_step = [&](const int ks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned so = row_of(8 * ks + e) * PLANE_ROW_BYTES;
            fa[ks][e] = ld_plane_nt(src, voff, so);
            fs[ks][e] = ld_plane_nt(src, voff, so + HID * PLANE_ROW_BYTES);
        }
    };
    auto split_step = [&](const int ks) {
        const float* __restrict__ L = p.Wt + OFF_L;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = fa[ks][e], s = fs[ks][e];
            if constexpr (HEAD) {                                // (k, s) -> (g_a, g_s): bwd_head_kernel's arithmetic, term for term
                const int c0 = (int)row_of(8 * ks + e);          // channel of lane-half 0; half 1: + 4
                const unsigned so = (unsigned)c0 * PLANE_ROW_BYTES;
                const float l0 = h ? L[c0 + 4] : L[c0], l1 = h ? L[HID + c0 + 4] : L[HID + c0], l2 = h ? L[2 * HID + c0 + 4] : L[2 * HID + c0];
                float g = l0 * go0;
                g = __builtin_fmaf(l1, go1, g);
                g = __builtin_fmaf(l2, go2, g);
                const float kv = a, sv = s;
                float sn, cs;
                dsincos(sv, sn, cs);
                a = kv > 0.0f ? g * sn : 0.0f;
                s = g * kv * cs;
                st_act(outQ_li, voff, so, kv * sn);
                st_act(outG_li, voff, so, a);
                st_act(outG_li, voff, so + HID * PLANE_ROW_BYTES, s);
            }
            __bf16 vh, vl;
            split2_bf16(a, vh, vl);
            gah[ks][e] = vh; gal[ks][e] = vl;
            split2_bf16(s, vh, vl);
            gsh[ks][e] = vh; gsl[ks][e] = vl;
        }
    };
#pragma unroll
    for (int ks = 0; ks < BLD; ++ks) load_step(ks);

    // A operand: the four pieces of a k-step by immediate offsets from one scalar offset
    constexpr int PF = 4;
    constexpr int KS_BYTES = (int)(WLX_KSTEP * sizeof(float));
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.split, 0, (int)(ST_FLOATS * sizeof(float)), 0x00020000);
    const int lane_off = lane * 16;
    const int wp = (int)((ST_OFF_BWD + (size_t)(li - 1) * WLX_LAYER) * sizeof(float));
    f32x4 rkh[PF], rqh[PF], rkl[PF], rql[PF];
    auto ld_kstep = [&](const int d, const int soff) {
        rkh[d] = ld_piece(wrs, lane_off, soff);
        rqh[d] = ld_piece(wrs, lane_off + 1 * PIECE_BYTES, soff);
        rkl[d] = ld_piece(wrs, lane_off + 2 * PIECE_BYTES, soff);
        rql[d] = ld_piece(wrs, lane_off + 3 * PIECE_BYTES, soff);
    };
#pragma unroll
    for (int d = 0; d < PF; ++d) ld_kstep(d, wp + d * KS_BYTES);

    // gates of layer li-1 for one finished element: g = d loss / d q_{li-1}[channel, pixel]
    auto gate_store = [&](int mt, int r, float g, float kv, float sv) {
        const unsigned so = (unsigned)(32 * mt + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES;
        float sn, cs;
        dsincos(sv, sn, cs);
        st_act(outG, voff, so, kv > 0.0f ? g * sn : 0.0f);
        st_act(outG, voff, so + HID * PLANE_ROW_BYTES, g * kv * cs);
        st_act(outQ, voff, so, kv * sn);
    };

    f32x16 pg;                                                   // finished g_q tile (sum of the two accumulators)
    float kt[16], st[16], ktn[16], stn[16];                      // saved k, s of the tile being finished / of the one in flight
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        f32x16 ak, as;
#pragma unroll
        for (int r = 0; r < 16; ++r) { ak[r] = 0.0f; as[r] = 0.0f; }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int s = m * 16 + ks;
            if (m == 0) split_step(ks);                           // (its loads went out BLD k-steps ago)
            const bf16x8 wkh = __builtin_bit_cast(bf16x8, rkh[s % PF]);
            const bf16x8 wqh = __builtin_bit_cast(bf16x8, rqh[s % PF]);
            // the two small products first, the leading one last (the forward's order)
            ak = MFMA_BF16(__builtin_bit_cast(bf16x8, rkl[s % PF]), gah[ks], ak);
            as = MFMA_BF16(__builtin_bit_cast(bf16x8, rql[s % PF]), gsh[ks], as);
            ak = MFMA_BF16(wkh, gal[ks], ak);
            as = MFMA_BF16(wqh, gsl[ks], as);
            ak = MFMA_BF16(wkh, gah[ks], ak);
            as = MFMA_BF16(wqh, gsh[ks], as);
            if (s + PF < 128) ld_kstep(s % PF, wp + (s + PF) * KS_BYTES);   // (a launch is one layer: nothing to fetch past its end,
                                                                             //  and layer 3's end is the image's end)
            if (m == 0 && ks + BLD < 16) load_step(ks + BLD);     // rest of the B operand, BLD k-steps ahead
            if (ks == 8) {                                        // saved planes of tile m, used from the next tile's first k-step on
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned so = (unsigned)(32 * m + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES;
                    ktn[r] = ld_plane_nt(act, voff, so);
                    stn[r] = ld_plane_nt(act, voff, so + HID * PLANE_ROW_BYTES);
                }
            }
            if (m > 0) gate_store(m - 1, ks, pg[ks], kt[ks], st[ks]);   // one epilogue element of tile m-1 per k-step
            __builtin_amdgcn_sched_barrier(0);                    // the region ends at the k-step
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pg[r] = ak[r] + as[r];
            kt[r] = ktn[r];
            st[r] = stn[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) gate_store(7, r, pg[r], kt[r], st[r]);
}

extern "C" {

int diinn_pack_split_train(void* stream, const float* image_dev, float* split_dev) {
    if (!image_dev || !split_dev) return DIINN_ERR_INVALID_ARG;
    if ((((size_t)image_dev) | ((size_t)split_dev)) & 15) return DIINN_ERR_INVALID_ARG;   // 16-byte loads and stores
    hipLaunchKernelGGL(split_train_pack_kernel, dim3(ST_PACK_THREADS / 256), dim3(256), 0, (hipStream_t)stream, image_dev, split_dev);
    return hip_status(hipGetLastError());
}

int diinn_backward_data_x3(void* stream, const float* gout_planes_dev, const float* acts_dev, const float* packed_dev,
                           const float* split_dev, float* G_dev, float* Q_dev, long long npix) {
    if (!gout_planes_dev || !acts_dev || !packed_dev || !split_dev || !G_dev || !Q_dev) return DIINN_ERR_INVALID_ARG;
    if (((size_t)split_dev) & 15) return DIINN_ERR_INVALID_ARG;  // 16-byte weight pieces
    const int stp = check_npix(npix);
    if (stp) return stp;
    BwdX3Params p;
    p.Wt = packed_dev; p.split = split_dev; p.acts = acts_dev; p.gout = gout_planes_dev; p.G = G_dev; p.Q = Q_dev;
    p.npix = npix; p.ntiles = (npix + PLANE_TILE - 1) / PLANE_TILE; p.layer = 0;
    const unsigned blocks = (unsigned)((p.ntiles + 3) / 4);
    for (int layer = 3; layer >= 1; --layer) {
        p.layer = layer;
        if (layer == 3) hipLaunchKernelGGL(bwd_layer_x3_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(bwd_layer_x3_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_status(e);
    }
    return DIINN_OK;
}

}  // extern "C"
