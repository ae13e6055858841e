// diinn_metasr_training.hip -- the MetaSR comparison decoder under autograd: the per-cell backward kernel
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h)
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// metasr_bwd_cells_kernel (training backward of metasr_kernel, reference metasr.py:70-104 under autograd).
// With W2r[n, comp, j] = imnet.layers.2.weight[3n + comp, j] the decoder is, per HR pixel p of LR cell c(p),
//     h = relu(a),  a = W1 (rel_h, rel_w, r_rev) + b1,     out[comp] = sum_j h_j M[c][comp][j] + B0[c][comp],
//     M[c][comp][j] = sum_n W2r[n, comp, j] U[c][n],       B0[c][comp] = sum_n b2[3n + comp] U[c][n],
// i.e. [M; B0] is a 3x3 convolution of the feature map with 771 outputs (the hoisted conv P under another weight), and the
// gradient at that convolution's output is a sum over the pixels of a cell:
//     dM[c][comp][j] = S = sum_p g_p[comp] h_p[j],          dB0[c][comp] = G = sum_p g_p[comp],
//     dh_p = sum_comp g_p[comp] M[c][comp][:],  da_p = dh_p [a_p > 0],  dW1 = sum_p da_p (x) (rel_h, rel_w, r_rev),  db1 = sum_p da_p.
// Everything wide (the 1728 x 256 layer, the unfold) then happens per cell on the kernels the DIINN training path has.
//
// One workgroup per plane tile of 32 consecutive flattened cells (b, cy, cx); thread = hidden channel j (256), the two halves
// of the workgroup take cells 0..15 and 16..31 of the tile.  MetaSR's index table is monotone, so a cell's pixels are the
// rectangle [seg_h[cy], seg_h[cy+1]) x [seg_w[cx], seg_w[cx+1]) (as for cell_sum_kernel); its pixels are walked rows first,
// then columns: a fixed order, no atomics -- two runs are bit-identical.  The pixel's coordinates and its three g values are
// uniform over the wave (scalar loads); a is recomputed with metasr_kernel's three fmaf in its order, so the mask is the
// forward's bit for bit.  A cell that owns no pixel (down-scaling) leaves zeros.
// The 771 sums of a cell go to LDS ([row][cell], pitch 33: the channel-strided writes and the cell-strided reads are both
// conflict-free); once the tile is complete the workgroup writes it in both of cell_sum_kernel's layouts, 32 lanes per row:
// tiled over cells [tile][1024][32] -- every 128-byte row of 32 cells leaves as one line -- and NCHW [B][1024][H][W].
// Rows 768..770 = G, rows 771..1023 = 0.  The layer-0 products leave as one [256][4] partial per half workgroup
// (columns rel_h, rel_w, r_rev, 1), added in order by diinn_sum_parts.
// Memory-bound: per cell 3 KiB of M read, 4 KiB + 4 KiB written (+ 12 B per pixel of g).
// ---------------------------------------------------------------------------------
constexpr int MB_ROWS = 3 * HID + 3;            // 771 rows of [S; G]
constexpr int MB_PITCH = PLANE_TILE + 1;

struct MetaBwdParams {
    const float* gout;       // [B,3,Hu,Wu]
    const float* M;          // [B,H,W,1024]: rows 256 comp + j (rows 768.. are not read)
    const float* Wt;         // MetaSR packed image (the MS_OFF_Q0 rows: W1 columns and b1)
    const int* seg_h;        // [H+1] first HR row of every LR row (seg_h[H] = Hu)
    const int* seg_w;        // [W+1]
    float* dM;               // [B][1024][H][W]
    float* dM_tiled;         // [ceil(B*H*W / 32)][1024][32]
    float* part0;            // [2 * tiles][256][4]
    int B, H, W, Hu, Wu;
    long long cells;
    MetaAxis ah, aw;
};

__global__ __launch_bounds__(512) void metasr_bwd_cells_kernel(const MetaBwdParams p) {
    __shared__ float stage[MB_ROWS * MB_PITCH];                       // 99.4 KiB
    const int j = threadIdx.x & (HID - 1);
    const int half = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    const long long tile = blockIdx.x;
    const int hw = p.H * p.W;
    const float* __restrict__ Q0 = p.Wt + MS_OFF_Q0;
    const float wh = Q0[0 * HID + j], ww = Q0[1 * HID + j], wr = Q0[2 * HID + j], b1 = Q0[3 * HID + j];
    const float a0 = __builtin_fmaf(wr, p.ah.r_rev, b1);
    const size_t plane = (size_t)p.Hu * p.Wu;
    float sh = 0.0f, sw = 0.0f, s1 = 0.0f;

#pragma unroll 1
    for (int i = 0; i < PLANE_TILE / 2; ++i) {
        const int s = half * (PLANE_TILE / 2) + i;
        const long long n = tile * PLANE_TILE + s;
        float S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, G0 = 0.0f, G1 = 0.0f, G2 = 0.0f;
        if (n < p.cells) {
            const int b = (int)(n / hw);
            const int rem = (int)(n - (long long)b * hw);
            const int cy = rem / p.W, cx = rem - cy * p.W;
            // (clamped: a bad table must not steer a load outside gout)
            const int y0 = max(p.seg_h[cy], 0), y1 = min(p.seg_h[cy + 1], p.Hu);
            const int x0 = max(p.seg_w[cx], 0), x1 = min(p.seg_w[cx + 1], p.Wu);
            if (y0 < y1 && x0 < x1) {
                const float* __restrict__ Mc = p.M + (size_t)n * PCH + j;
                const float m0 = Mc[0], m1 = Mc[HID], m2 = Mc[2 * HID];
                const float* __restrict__ gb = p.gout + (size_t)b * 3 * plane;
                for (int y = y0; y < y1; ++y) {
                    int iy;
                    float relh;
                    meta_axis_eval(p.ah, y, iy, relh);
                    const float* __restrict__ gr = gb + (size_t)y * p.Wu;
                    for (int x = x0; x < x1; ++x) {
                        int ix;
                        float relw;
                        meta_axis_eval(p.aw, x, ix, relw);
                        const float g0 = gr[x], g1 = gr[plane + x], g2 = gr[2 * plane + x];
                        float a = __builtin_fmaf(ww, relw, a0);
                        a = __builtin_fmaf(wh, relh, a);
                        const float hj = relu0(a);
                        const float dh = __builtin_fmaf(g2, m2, __builtin_fmaf(g1, m1, g0 * m0));
                        const float da = a > 0.0f ? dh : 0.0f;
                        S0 = __builtin_fmaf(g0, hj, S0);
                        S1 = __builtin_fmaf(g1, hj, S1);
                        S2 = __builtin_fmaf(g2, hj, S2);
                        G0 += g0;
                        G1 += g1;
                        G2 += g2;
                        sh = __builtin_fmaf(da, relh, sh);
                        sw = __builtin_fmaf(da, relw, sw);
                        s1 += da;
                    }
                }
            }
        }
        stage[(0 * HID + j) * MB_PITCH + s] = S0;
        stage[(1 * HID + j) * MB_PITCH + s] = S1;
        stage[(2 * HID + j) * MB_PITCH + s] = S2;
        if (j < 3) stage[(3 * HID + j) * MB_PITCH + s] = j == 0 ? G0 : (j == 1 ? G1 : G2);
    }
    *(f32x4*)(p.part0 + (((size_t)tile * 2 + half) * HID + j) * 4) = f32x4{sh, sw, s1 * p.ah.r_rev, s1};
    __syncthreads();

    // the tile in both layouts: 32 lanes per row, 16 rows per pass
    const int s = threadIdx.x & (PLANE_TILE - 1);
    const long long n = tile * PLANE_TILE + s;
    const bool live = n < p.cells;
    const int b = live ? (int)(n / hw) : 0;
    const int rem = live ? (int)(n - (long long)b * hw) : 0;
    float* __restrict__ dt = p.dM_tiled + (size_t)tile * PCH * PLANE_TILE + s;
    float* __restrict__ dn = p.dM + (size_t)b * PCH * hw + rem;
#pragma unroll 4
    for (int r = (int)(threadIdx.x >> 5); r < PCH; r += 16) {
        const float v = r < MB_ROWS ? stage[r * MB_PITCH + s] : 0.0f;
        dt[(size_t)r * PLANE_TILE] = live ? v : 0.0f;
        if (live) dn[(size_t)r * hw] = v;
    }
}

extern "C" {

int diinn_metasr_backward_cells(void* stream, const float* gout_dev, const float* M_dev, const float* packed_dev,
                                const int32_t* seg_h_dev, const int32_t* seg_w_dev, float* dM_dev, float* dM_tiled_dev,
                                float* part0_dev, int B, int H, int W, int Hu, int Wu) {
    if (!gout_dev || !M_dev || !packed_dev || !seg_h_dev || !seg_w_dev || !dM_dev || !dM_tiled_dev || !part0_dev)
        return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    st = check_npix((long long)B * Hu * Wu);
    if (st) return st;
    if ((long long)H * W > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    if (((size_t)part0_dev) & 15) return DIINN_ERR_INVALID_ARG;          // 16-byte stores of the layer-0 partials
    const long long cells = (long long)B * H * W;
    const long long tiles = (cells + PLANE_TILE - 1) / PLANE_TILE;
    if (tiles > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    MetaBwdParams p;
    p.gout = gout_dev; p.M = M_dev; p.Wt = packed_dev; p.seg_h = seg_h_dev; p.seg_w = seg_w_dev;
    p.dM = dM_dev; p.dM_tiled = dM_tiled_dev; p.part0 = part0_dev;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu; p.cells = cells;
    p.ah = make_meta_axis(H, Hu);
    p.aw = make_meta_axis(W, Wu);
    hipLaunchKernelGGL(metasr_bwd_cells_kernel, dim3((unsigned)tiles), dim3(512), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

}  // extern "C"
