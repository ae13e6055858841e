// diinn_initq_training.hip -- decoder init_q=True, mode 3, under autograd: what the backward pass adds to diinn_training.hip
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, image and plane layout in diinn_layout.h)
//
// Reference path replaced: autograd through ImplicitDecoder.step with init_q (diinn.py:48-51,113-115,132-139).  Per HR pixel
//   a = Fw syn + bF,  E = sin a,  x' = E * X[cell],  k_i = relu(Wq_i q_{i-1} + Wx_i x' + bK_i),  s_0 = Q0 E + bQ0,
// and bwd_layer_kernel (diinn_backward_data) leaves the gate gradients G_i = (g_a,i ; g_s,i) as for mode 3.  New here:
//   dx' = sum_i Wx_i^T g_a,i      t = Q0^T g_s,0      U = dx' * E      da = (dx' * X + t) * cos a
//   initq_bwd_kernel      the two transposed per-pixel GEMMs and their epilogue: writes U, da, x', E as tiled groups
//   cell_sum_rows_kernel  dXunf[b, n, cy, cx] = sum of U[n] over the HR pixels of LR cell (cy, cx)   (cell_sum_kernel for one group of R rows)
//   fold3x3_kernel        dfeat = fold3x3(dXunf): the adjoint of unfold3x3
// The parameter gradients are the library's plane GEMM and rowdot over x', E, da (initq_training.py).
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// initq_bwd_kernel: D1 [640 x pixels] = WxT [640 x 1024] . (g_a,0 ; .. ; g_a,3)   and   D2 = Q0T [640 x 256] . g_s,0
// on v_mfma_f32_32x32x2_f32 (rows 576..639 are zero padding: 20 M-tiles, 5 per wave).
// Workgroup = 4 waves = 64 pixels = two plane tiles = two N-tiles.  The reduction runs in five CHUNKS of 256 rows (the g_a rows of
// G_0..G_3, then the g_s rows of G_0); a chunk of both tiles, 2 x 256 rows x 128 B = 64 KiB, is copied ONCE per workgroup into LDS
// as 64 coalesced 1 KiB LDS-DMA pieces (16 per wave, no registers), two stages.  A row of a tile is 128 contiguous bytes and the
// MFMA's k pair is two neighbouring rows, so the B operand of k-step kk is the 256 contiguous bytes at row 2 kk: one conflict-free
// ds_read_b32 at an immediate offset.  A wave owns 5 M-tiles; all of them x 2 N-tiles x (D1, D2) would be 320 accumulator
// registers, more than either half of the register file holds, so it walks the reduction TWICE -- M-tiles 0..2 (192 accumulators),
// then 3..4 (128) -- and the workgroup stages G twice (5,120 bytes per pixel and pass, against 9,728 written).  Its weight pieces
// (section WT of the training image, contiguous per wave in the order it consumes them) arrive through a register ring two
// k-groups deep: a 1 KiB piece feeds 8 MFMAs, a k-group's 8 B values feed 24 or 16.
// Epilogue, per accumulator element (row n, pixel): a, E = sin a, cos a with the forward's operation order (fma(Fr, ratio, bF), then
// rel_w, then rel_h; axis_eval for the cell), X by the forward's clamped load and select; U, da (576 rows), x', E (640 rows, the
// padding rows written as zeros: diinn_plane_gemm_nt wants M % 128 == 0).
// A pixel is one column of the GEMM: the columns of a ragged last tile's padding (never written by bwd_layer_kernel) meet no other
// column and are not stored.  No atomics, no scratch, fixed summation order, one workgroup per CU.
// ---------------------------------------------------------------------------------
struct InitqBwdParams {
    const float* feat;       // [B,64,H,W]
    const float* G;          // tiled [4][ntiles][512][32]
    const float* img;        // the init_q training image (diinn_pack_initq_train)
    float* U;                // tiled [ntiles][576][32]   dx' * E
    float* dA;               // tiled [ntiles][576][32]   d loss / d a
    float* XP;               // tiled [ntiles][640][32]   x' (rows 576.. zero)
    float* E;                // tiled [ntiles][640][32]   E  (rows 576.. zero)
    long long npix, ntiles;
    int B, H, W, Hu, Wu;
    float ratio;
    Axis ah, aw;
};

constexpr int IB_TILE_FLOATS = HID * PLANE_TILE;                 // one tile's 256 rows of a chunk: 8,192 floats = 32 KiB
constexpr int IB_STAGE_FLOATS = 2 * IB_TILE_FLOATS;              // 64 KiB

__device__ __forceinline__ void iq_sincos(float x, float& sn, float& cs) {   // dsin<DIINN_SIN_HW_REDUCED>'s reduction, sine and cosine
    constexpr float C_HI = 0.15915494309189533577f;
    constexpr float C_LO = 6.4206383650924e-09f;
    const float k = __builtin_rintf(x * C_HI);
    float r = __builtin_fmaf(x, C_HI, -k);
    r = __builtin_fmaf(x, C_LO, r);
    sn = __builtin_amdgcn_sinf(r);
    cs = __builtin_amdgcn_cosf(r);
}

__global__ __launch_bounds__(256, 1) void initq_bwd_kernel(const InitqBwdParams p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * IB_STAGE_FLOATS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const long long tile0 = (long long)blockIdx.x * 2;
    const size_t agroup = (size_t)p.ntiles * ACT_ROWS * PLANE_TILE;

    // this wave's k-th piece (0..15) of chunk c into stage st: piece 16 wave + k = (N-tile, rows 8 r .. 8 r + 7)
    auto dma_piece = [&](int st, int c, int k) {
        const int i = 16 * wave + k;
        const int nt = i >> 5, r8 = i & 31;
        const long long tile = tile0 + nt;
        const float* src = p.G + (size_t)(c < 4 ? c : 0) * agroup + (size_t)(tile < p.ntiles ? tile : 0) * (ACT_ROWS * PLANE_TILE) +
                           (c < 4 ? 0 : HID * PLANE_TILE);
        // a tile past the end: an empty descriptor, the loads return zeros
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, tile < p.ntiles ? HID * (int)PLANE_ROW_BYTES : 0,
                                                                            0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + st * IB_STAGE_FLOATS + i * 256), 16,
                                                 lane * 16, r8 * 1024, 0, 0);
    };

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.img + IQT_OFF_WT + (size_t)wave * IQT_WAVE), 0, (int)(IQT_WAVE * sizeof(float)), 0x00020000);   // reads past the end return 0
    const int lane_off = lane * 16;
    const float* __restrict__ F = p.img + IQ_OFF_F;
    const int hw = p.Hu * p.Wu;
#pragma unroll
    for (int k = 0; k < 16; ++k) dma_piece(0, 0, k);

    // One pass: NM of the wave's M-tiles (from M-tile mt0 of its five) against the whole reduction, then their epilogue.
    // `gc0` counts the chunks staged before the pass (the stage of chunk c is (gc0 + c) & 1); `wbase` is the pass's byte offset in
    // the wave's weight stream, [chunk][kg][mt NM] pieces.
    auto run_pass = [&](auto nm_c, const int mt0, const int gc0, const int wbase, const bool last_pass) {
        constexpr int NM = decltype(nm_c)::value;
        f32x16 accx[NM][2], acct[NM][2];
#pragma unroll
        for (int mt = 0; mt < NM; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { accx[mt][nt][r] = 0.0f; acct[mt][nt][r] = 0.0f; }
        f32x4 rw[2][NM];                                         // the pieces of two k-groups: a piece arrives 2 x 8 NM MFMAs ahead
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int mt = 0; mt < NM; ++mt) rw[u][mt] = ld_piece(wrs, lane_off, wbase + (u * NM + mt) * PIECE_BYTES);

        // one chunk: [own pieces landed] -> barrier (everybody's landed; everybody is done with the other stage) -> the next
        // chunk's pieces go out one per k-group behind the MFMAs -> 32 k-groups x 8 NM MFMAs
        auto run_chunk = [&](const int c, f32x16 (&acc)[NM][2]) {
            const int st = (gc0 + c) & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const bool more = !(last_pass && c + 1 == IQT_CHUNKS);
            const int cn = c + 1 < IQT_CHUNKS ? c + 1 : 0;       // the chunk staged next (the next pass starts over at chunk 0)
            const float* bm = lds + st * IB_STAGE_FLOATS + lane;
#pragma unroll 1
            for (int kg2 = 0; kg2 < IQT_KG / 2; ++kg2) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int kg = 2 * kg2 + u;
                    float b0[4], b1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        b0[e] = bm[64 * (4 * kg + e)];
                        b1[e] = bm[IB_TILE_FLOATS + 64 * (4 * kg + e)];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int mt = 0; mt < NM; ++mt) {
                            acc[mt][0] = MFMA32(rw[u][mt][e], b0[e], acc[mt][0]);
                            acc[mt][1] = MFMA32(rw[u][mt][e], b1[e], acc[mt][1]);
                        }
                    const int s = (c * IQT_KG + kg + 2) * NM;    // two k-groups ahead (past the pass's last: never used)
#pragma unroll
                    for (int mt = 0; mt < NM; ++mt) rw[u][mt] = ld_piece(wrs, lane_off, wbase + (s + mt) * PIECE_BYTES);
                }
                if (more && kg2 < 16) dma_piece(st ^ 1, cn, kg2);
            }
        };
#pragma unroll 1
        for (int c = 0; c < 4; ++c) run_chunk(c, accx);
        run_chunk(4, acct);

        // ---- epilogue of the pass's M-tiles
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const long long tile = tile0 + nt;
            if (tile >= p.ntiles) continue;                      // wave-uniform
            const long long pix = tile * PLANE_TILE + j;
            const bool valid = pix < p.npix;
            const long long pc = valid ? pix : p.npix - 1;       // lanes past the end compute on the last pixel and store nothing
            const int b = (int)(pc / hw);
            const int rem = (int)(pc - (long long)b * hw);
            const int y = rem / p.Wu, x = rem - y * p.Wu;
            int iy, ix;
            float relh, relw;
            axis_eval(p.ah, y, iy, relh);
            axis_eval(p.aw, x, ix, relw);
            const float* __restrict__ fb = p.feat + (size_t)b * C_IN * p.H * p.W;
            const unsigned voff = valid ? 4u * j + 4u * h * PLANE_ROW_BYTES : 0xFFFFFFF0u;
            const __amdgpu_buffer_rsrc_t rU = tile_rsrc(p.U, tile, UNF), rA = tile_rsrc(p.dA, tile, UNF);
            const __amdgpu_buffer_rsrc_t rX = tile_rsrc(p.XP, tile, IQT_ROWS), rE = tile_rsrc(p.E, tile, IQT_ROWS);
#pragma unroll
            for (int mt = 0; mt < NM; ++mt) {
                const int mtg = IQT_MT * wave + mt0 + mt;        // wave-uniform
                if (mtg >= UNF / 32) {                           // the padding rows 576..639 of x' and E
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned so = (unsigned)(32 * mtg + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES;
                        st_act(rX, voff, so, 0.0f);
                        st_act(rE, voff, so, 0.0f);
                    }
                    continue;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n0 = 32 * mtg + (r & 3) + 8 * (r >> 2);   // the row of lane-half 0 (wave-uniform); half 1: + 4
                    const int n = n0 + 4 * h;
                    float a = __builtin_fmaf(F[2 * UNF + n], p.ratio, F[3 * UNF + n]);
                    a = __builtin_fmaf(F[1 * UNF + n], relw, a);
                    a = __builtin_fmaf(F[0 * UNF + n], relh, a);
                    float sn, cs;
                    iq_sincos(a, sn, cs);
                    const int c = n / 9, tap = n - 9 * c;
                    const int ky = tap / 3, kx = tap - 3 * ky;
                    const int yy = iy + ky - 1, xx = ix + kx - 1;
                    const bool ok = (yy >= 0) && (yy < p.H) && (xx >= 0) && (xx < p.W);
                    const int yc = yy < 0 ? 0 : (yy >= p.H ? p.H - 1 : yy);
                    const int xc = xx < 0 ? 0 : (xx >= p.W ? p.W - 1 : xx);
                    const float v = fb[((size_t)c * p.H + yc) * p.W + xc];
                    const float X = ok ? v : 0.0f;
                    const float dx = accx[mt][nt][r];
                    const float de = __builtin_fmaf(dx, X, acct[mt][nt][r]);
                    const unsigned so = (unsigned)n0 * PLANE_ROW_BYTES;
                    st_act(rU, voff, so, dx * sn);
                    st_act(rA, voff, so, de * cs);
                    st_act(rX, voff, so, sn * X);
                    st_act(rE, voff, so, sn);
                }
            }
        }
    };
    run_pass(IC<IQT_MT_A>{}, 0, 0, 0, false);
    run_pass(IC<IQT_MT - IQT_MT_A>{}, IQT_MT_A, IQT_CHUNKS, (int)(IQT_PASS_B * sizeof(float)), true);
}

// ---------------------------------------------------------------------------------
// cell_sum_rows_kernel: cell_sum_kernel (diinn_training.hip) for ONE tiled group of `rows` rows per tile, of which rows [0, R) are
// summed: out[b, n, cy, cx] = sum of row n over the HR pixels of LR cell (cy, cx), NCHW [B][R][H][W].  The same seg tables, the same
// summation order (left to right inside a row, rows top to bottom), the same wide loads at the integer scales; a cell that owns no
// pixel (down-scaling) gets zero.
// ---------------------------------------------------------------------------------
struct CellSumRowsParams {
    const float* G;          // tiled [ntiles][rows][32]
    float* out;              // [B][R][H][W]
    const int* seg_h;        // [H+1]
    const int* seg_w;        // [W+1]
    int B, H, W, Hu, Wu, rows, R;
};

__global__ __launch_bounds__(256) void cell_sum_rows_kernel(const CellSumRowsParams p) {
    const int cell = blockIdx.x * 256 + threadIdx.x;                 // cy * W + cx
    if (cell >= p.H * p.W) return;
    const int b = blockIdx.y;
    const int cy = cell / p.W, cx = cell - cy * p.W;
    const int plane = blockIdx.z;
    const float* __restrict__ src = p.G + (size_t)plane * PLANE_TILE;
    const size_t tstride = (size_t)p.rows * PLANE_TILE;
    const int y0 = p.seg_h[cy], y1 = p.seg_h[cy + 1];
    const int x0 = p.seg_w[cx], x1 = p.seg_w[cx + 1];
    const int wd = x1 - x0;
    auto at = [&](long long pix) { return src + (size_t)(pix >> 5) * tstride + (size_t)(pix & 31); };
    float acc = 0.0f;
    if (wd == 4 && ((p.Wu | x0) & 3) == 0) {                     // (the 4 pixels lie in one tile row, 16-byte aligned: cell_sum_kernel)
        for (int y = y0; y < y1; y += 4) {
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (y + k < y1) v[k] = __builtin_nontemporal_load((const f32x4*)at(((long long)b * p.Hu + y + k) * p.Wu + x0));
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (y + k < y1) acc += ((v[k][0] + v[k][1]) + v[k][2]) + v[k][3];
        }
    } else if (wd == 2 && ((p.Wu | x0) & 1) == 0) {
        for (int y = y0; y < y1; y += 4) {
            f32x2 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (y + k < y1) v[k] = *(const f32x2*)at(((long long)b * p.Hu + y + k) * p.Wu + x0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (y + k < y1) acc += v[k][0] + v[k][1];
        }
    } else {
        for (int y = y0; y < y1; ++y) {
            const long long rowpix = ((long long)b * p.Hu + y) * p.Wu;
            float r = 0.0f;
            for (int x = x0; x < x1; ++x) r += *at(rowpix + x);
            acc += r;
        }
    }
    p.out[(((size_t)b * p.R + plane) * p.H + cy) * p.W + cx] = acc;
}

// ---------------------------------------------------------------------------------
// fold3x3_kernel: the adjoint of the reference's F.unfold(feat, 3, padding=1) (diinn.py:168; row n = c * 9 + 3 ky + kx):
//   dfeat[b, c, y, x] = sum over ky, kx of dXunf[b, 9 c + 3 ky + kx, y - ky + 1, x - kx + 1],  terms outside the map dropped.
// One thread per output element, the nine terms added in (ky, kx) order.  HBM-bound (reads dXunf once).
// ---------------------------------------------------------------------------------
struct FoldParams {
    const float* d;          // [B][9 C][H][W]
    float* out;              // [B][C][H][W]
    int B, C, H, W;
};

__global__ __launch_bounds__(256) void fold3x3_kernel(const FoldParams p) {
    const int cell = blockIdx.x * 256 + threadIdx.x;                 // y * W + x
    if (cell >= p.H * p.W) return;
    const int y = cell / p.W, x = cell - y * p.W;
    const int c = blockIdx.y, b = blockIdx.z;
    const size_t hw = (size_t)p.H * p.W;
    const float* __restrict__ src = p.d + ((size_t)b * p.C + c) * 9 * hw;
    float acc = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y - ky + 1, xx = x - kx + 1;
            if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) acc += src[(size_t)(3 * ky + kx) * hw + (size_t)yy * p.W + xx];
        }
    p.out[((size_t)b * p.C + c) * hw + cell] = acc;
}

extern "C" {

int diinn_initq_backward(void* stream, const float* feat_dev, const float* G_dev, const float* train_image_dev,
                         float* U_dev, float* dA_dev, float* XP_dev, float* E_dev, int B, int H, int W, int Hu, int Wu) {
    if (!feat_dev || !G_dev || !train_image_dev || !U_dev || !dA_dev || !XP_dev || !E_dev) return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if ((double)Hu * Wu >= 2.0e9) return DIINN_ERR_TOO_LARGE;
    const long long npix = (long long)B * Hu * Wu;
    st = check_npix(npix);
    if (st) return st;
    // 16-byte pieces of G and of the image
    if ((((size_t)G_dev) | ((size_t)train_image_dev)) & 15) return DIINN_ERR_INVALID_ARG;
    InitqBwdParams p;
    p.feat = feat_dev; p.G = G_dev; p.img = train_image_dev; p.U = U_dev; p.dA = dA_dev; p.XP = XP_dev; p.E = E_dev;
    p.npix = npix; p.ntiles = (npix + PLANE_TILE - 1) / PLANE_TILE;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu;
    p.ratio = (float)(((double)H * (double)W) / ((double)Hu * (double)Wu));
    const int small = diinn_uses_small_output_kernel(Hu, Wu);
    p.ah = make_axis(H, Hu, small);
    p.aw = make_axis(W, Wu, small);
    if ((p.ntiles + 1) / 2 > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    hipLaunchKernelGGL(initq_bwd_kernel, dim3((unsigned)((p.ntiles + 1) / 2)), dim3(256), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

int diinn_cell_sum_rows(void* stream, const float* group_dev, int rows, int R, const int32_t* seg_h_dev, const int32_t* seg_w_dev,
                        float* out_dev, int B, int H, int W, int Hu, int Wu) {
    if (!group_dev || !seg_h_dev || !seg_w_dev || !out_dev) return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0 || R <= 0 || R > rows) return DIINN_ERR_INVALID_ARG;
    st = check_npix((long long)B * Hu * Wu);
    if (st) return st;
    if (B > 65535 || R > 65535 || (long long)H * W > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    if (((size_t)group_dev) & 15) return DIINN_ERR_INVALID_ARG;
    CellSumRowsParams p{group_dev, out_dev, seg_h_dev, seg_w_dev, B, H, W, Hu, Wu, rows, R};
    hipLaunchKernelGGL(cell_sum_rows_kernel, dim3((unsigned)(((long long)H * W + 255) / 256), (unsigned)B, (unsigned)R), dim3(256), 0,
                       (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

int diinn_fold3x3(void* stream, const float* dxunf_dev, float* dfeat_dev, int B, int C, int H, int W) {
    if (!dxunf_dev || !dfeat_dev) return DIINN_ERR_INVALID_ARG;
    const int st = check_dims(B, H, W);
    if (st) return st;
    if (C <= 0) return DIINN_ERR_INVALID_ARG;
    if (C > 65535 || (long long)H * W > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    FoldParams p{dxunf_dev, dfeat_dev, B, C, H, W};
    hipLaunchKernelGGL(fold3x3_kernel, dim3((unsigned)(((long long)H * W + 255) / 256), (unsigned)C, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

}  // extern "C"
