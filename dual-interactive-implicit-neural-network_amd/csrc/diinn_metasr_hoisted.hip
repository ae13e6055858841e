// diinn_metasr_hoisted.hip -- the MetaSR comparison decoder in its hoisted form: pixels from the per-cell conv [M; B0]
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h)
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// metasr_hoisted_kernel (the forward that diinn_metasr_training.hip's header states; reference metasr.py:70-104).
// With [M; B0][c] = conv3x3(feat; W2r, b2r) per LR cell (diinn_precompute_P_wpu on the MetaSR training image), an HR pixel
// p of cell c(p) is
//     h = relu(a),  a = W1 (rel_h, rel_w, r_rev) + b1,     out[comp] = sum_j h_j M[c][comp][j] + B0[c][comp]:
// 256 hidden values and 771 FMAs per pixel (~3.6 kFLOP) instead of metasr_kernel's 885 kFLOP.
//
// One workgroup per block of 16 x 16 HR pixels, lane = pixel, wave = 16 x 4 pixels.  The pixel's cell and (rel_h, rel_w) are
// meta_axis_eval's -- metasr_kernel's, bit for bit -- and a_j is its three fmaf in its order, so the ReLU mask is the one
// metasr_bwd_cells_kernel recomputes.  The W1 / b1 rows are uniform over the wave (scalar loads).  Per comp the sum runs over
// j = 0..255 in order into one accumulator, then + B0: fixed order, no atomics -- two runs are bit-identical, and so are the
// two paths below (the same FMAs on the same values).  Lanes past the right edge or the end of the row window compute on a
// clamped pixel and skip the store.
//
// Staged path (up-scaling).  meta_axis_eval is monotone in the pixel index, so the cells of a block are the rectangle between
// the cells of its first and last (clamped) row and column.  When that rectangle has at most MH_MAX_CELLS cells, their M
// rows go through LDS in chunks of jc = 128 / 64 / 32 hidden channels (the largest that fits the rectangle into MH_LDS
// floats): consecutive threads copy consecutive 16 bytes of a cell's [comp][jc] rows -- coalesced, up to 12 loads per thread in
// flight before the first store -- and after a barrier every lane reads its own cell's values from LDS (lanes that share a cell
// read one address: a broadcast).  Every M value is loaded once per workgroup: at x4 a block holds all 16 pixels of each of
// its 16 cells, so it leaves HBM once (a block that straddles cell borders re-reads a border cell that a neighbour has just
// pulled into the L2 / Infinity Cache).
// LDS: [cell][comp][jc + 4] floats (the 4 floats of padding stagger the cells over the banks), 48 KiB, three workgroups per CU.
// Direct path (more cells than that: scales below ~1.5, down-scaling; or a lane outside the rectangle, which the
// monotone table rules out).  Every lane reads its own cell's values from global memory, 16 bytes at a time, eight j ahead of
// the FMAs.  Correct for every geometry; the vector memory unit takes 64 addresses per instruction whether or not they
// coincide, so where lanes share cells this path is bound by that rate, not by bytes (measured: DESIGN.md section 3.8).
// Per cell 3,084 B of M read, per pixel 12 B written (rows 771..1023 of a cell are not read).
// ---------------------------------------------------------------------------------
constexpr int MH_BLOCK_W = 16;                  // HR pixels of a workgroup along x (= of a wave)
constexpr int MH_WAVE_H = 4;                    // HR rows of a wave
constexpr int MH_BLOCK_H = 4 * MH_WAVE_H;       // 4 waves
constexpr int MH_CHUNK = 8;                     // direct path: hidden channels per load batch (6 x 16 bytes per lane)
constexpr int MH_LDS = 12288;                   // staged path: floats of LDS (48 KiB)
constexpr int MH_PAD = 4;                       // floats of padding behind each [jc] row
constexpr int MH_MAX_CELLS = MH_LDS / (3 * (32 + MH_PAD));      // 113: the rectangle still fits at jc = 32
constexpr int MH_COPIES = MH_LDS / 4 / 256;     // 12: 16-byte pieces of a chunk per thread, at most

struct MetaHoistParams {
    const float* M;          // [B,H,W,1024]: rows 256 comp + j = M, rows 768 + comp = B0
    const float* Wt;         // MetaSR packed image (the MS_OFF_Q0 rows: W1 columns and b1)
    float* out;              // [B,3,Hu,Wu]
    int B, H, W, Hu, Wu, y0, y1;
    MetaAxis ah, aw;
};

// The W1 / b1 rows are read-only for the kernel's lifetime and their index is uniform over the wave: read through the constant
// address space they stay scalar loads (behind the LDS stores and barriers of the staged path the compiler no longer proves
// that by itself and falls back to 64 identical vector loads per value).
typedef const __attribute__((address_space(4))) float* mh_const_ptr;

// acc[comp] += sum over the 8 hidden channels j0 .. j0 + 7 of relu(a_j) m[comp][j], j ascending
__device__ __forceinline__ void mh_fma8(mh_const_ptr Q0, int j0, float r_rev, float relh, float relw,
                                        const f32x4 (&m)[3][2], float& acc0, float& acc1, float& acc2) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = j0 + e;
        float a = __builtin_fmaf(Q0[2 * HID + j], r_rev, Q0[3 * HID + j]);
        a = __builtin_fmaf(Q0[1 * HID + j], relw, a);
        a = __builtin_fmaf(Q0[0 * HID + j], relh, a);
        const float hj = relu0(a);
        acc0 = __builtin_fmaf(hj, m[0][e >> 2][e & 3], acc0);
        acc1 = __builtin_fmaf(hj, m[1][e >> 2][e & 3], acc1);
        acc2 = __builtin_fmaf(hj, m[2][e >> 2][e & 3], acc2);
    }
}

__device__ __forceinline__ void mh_load(const float* __restrict__ Mc, int j0, f32x4 (&m)[3][2]) {
#pragma unroll
    for (int comp = 0; comp < 3; ++comp)
#pragma unroll
        for (int q = 0; q < 2; ++q) m[comp][q] = *(const f32x4*)(Mc + comp * HID + j0 + 4 * q);
}

__global__ __launch_bounds__(256) void metasr_hoisted_kernel(const MetaHoistParams p) {
    __shared__ __attribute__((aligned(16))) float stage[MH_LDS];
    __shared__ int cell_of[MH_MAX_CELLS];                        // staged path: (cy * W + cx) of the rectangle's cells
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int bx0 = blockIdx.x * MH_BLOCK_W;
    const int by0 = p.y0 + blockIdx.y * MH_BLOCK_H;              // < y1: the grid covers the window and no more
    const int x = bx0 + (lane & (MH_BLOCK_W - 1));
    const int y = by0 + wave * MH_WAVE_H + (lane >> 4);
    const int b = blockIdx.z;
    const bool valid = (x < p.Wu) && (y < p.y1);
    const int xc = x < p.Wu ? x : p.Wu - 1;
    const int yc = y < p.y1 ? y : p.y1 - 1;
    int iy, ix;
    float relh, relw;
    meta_axis_eval(p.ah, yc, iy, relh);
    meta_axis_eval(p.aw, xc, ix, relw);
    const mh_const_ptr Q0 = (mh_const_ptr)(p.Wt + MS_OFF_Q0);
    const float r_rev = p.ah.r_rev;
    const float* __restrict__ Mb = p.M + (size_t)b * p.H * p.W * PCH;
    const float* __restrict__ Mc = Mb + ((size_t)iy * p.W + ix) * PCH;

    // the block's cell rectangle (uniform over the workgroup)
    int cy_lo, cy_hi, cx_lo, cx_hi;
    {
        float unused;
        const int y_last = by0 + MH_BLOCK_H - 1 < p.y1 ? by0 + MH_BLOCK_H - 1 : p.y1 - 1;
        const int x_last = bx0 + MH_BLOCK_W - 1 < p.Wu ? bx0 + MH_BLOCK_W - 1 : p.Wu - 1;
        meta_axis_eval(p.ah, by0, cy_lo, unused);
        meta_axis_eval(p.ah, y_last, cy_hi, unused);
        meta_axis_eval(p.aw, bx0, cx_lo, unused);
        meta_axis_eval(p.aw, x_last, cx_hi, unused);
    }
    const int ncy = cy_hi - cy_lo + 1, ncx = cx_hi - cx_lo + 1;
    const bool fits = ncy >= 1 && ncx >= 1 && ncy <= MH_MAX_CELLS && ncx <= MH_MAX_CELLS && ncy * ncx <= MH_MAX_CELLS;
    const int ly = iy - cy_lo, lx = ix - cx_lo;
    const bool inside = ly >= 0 && ly < ncy && lx >= 0 && lx < ncx;
    const bool staged = fits && !__syncthreads_or((int)!inside);

    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
    if (staged) {
        const int ncell = ncy * ncx;                             // <= MH_MAX_CELLS
        const int jc = ncell * 3 * (128 + MH_PAD) <= MH_LDS ? 128 : (ncell * 3 * (64 + MH_PAD) <= MH_LDS ? 64 : 32);
        const int pitch = jc + MH_PAD;                           // ncell * 3 * pitch <= MH_LDS by the choice of jc
        const int qshift = jc == 128 ? 5 : (jc == 64 ? 4 : 3);   // log2 of the 16-byte pieces of a [jc] row
        const float* __restrict__ mine = stage + (ly * ncx + lx) * 3 * pitch;
        if ((int)threadIdx.x < ncell) {
            const int ccy = (int)threadIdx.x / ncx, ccx = (int)threadIdx.x - ccy * ncx;
            cell_of[threadIdx.x] = (cy_lo + ccy) * p.W + (cx_lo + ccx);      // (H * W < 2^31: the launch function)
        }
        __syncthreads();
        const int nv = ncell * 3 << qshift;                      // 16-byte pieces of a chunk: <= MH_LDS / 4
#pragma unroll 1
        for (int jc0 = 0; jc0 < HID; jc0 += jc) {
            if (jc0) __syncthreads();                            // everyone is done with the previous chunk
            // piece v = (cell, comp, q): consecutive threads take consecutive 16 bytes of a cell's [jc] row; all loads, then all stores
            f32x4 r[MH_COPIES];
#pragma unroll
            for (int i = 0; i < MH_COPIES; ++i) {
                // (past the end: the last piece again, loaded and not stored: no branch between the loads)
                const int v = (int)threadIdx.x + 256 * i < nv ? (int)threadIdx.x + 256 * i : nv - 1;
                const int row = v >> qshift, q = v - (row << qshift);
                const int c = row / 3, comp = row - 3 * c;
                r[i] = *(const f32x4*)(Mb + (size_t)cell_of[c] * PCH + comp * HID + jc0 + 4 * q);
            }
#pragma unroll
            for (int i = 0; i < MH_COPIES; ++i) {
                const int v = (int)threadIdx.x + 256 * i;
                if (v < nv) {
                    const int row = v >> qshift, q = v - (row << qshift);
                    *(f32x4*)(stage + row * pitch + 4 * q) = r[i];
                }
            }
            __syncthreads();
#pragma unroll 2
            for (int jj = 0; jj < jc; jj += 8) {
                f32x4 m[3][2];
#pragma unroll
                for (int comp = 0; comp < 3; ++comp)
#pragma unroll
                    for (int q = 0; q < 2; ++q) m[comp][q] = *(const f32x4*)(mine + comp * pitch + jj + 4 * q);
                mh_fma8(Q0, jc0 + jj, r_rev, relh, relw, m, acc0, acc1, acc2);
            }
        }
    } else {
        f32x4 cur[3][2], nxt[3][2];
        mh_load(Mc, 0, cur);
#pragma unroll 2
        for (int j0 = 0; j0 < HID; j0 += MH_CHUNK) {
            mh_load(Mc, j0 + MH_CHUNK < HID ? j0 + MH_CHUNK : j0, nxt);        // (the last batch is loaded twice, not past the rows)
            mh_fma8(Q0, j0, r_rev, relh, relw, cur, acc0, acc1, acc2);
#pragma unroll
            for (int comp = 0; comp < 3; ++comp)
#pragma unroll
                for (int q = 0; q < 2; ++q) cur[comp][q] = nxt[comp][q];
        }
    }
    acc0 += Mc[3 * HID + 0];
    acc1 += Mc[3 * HID + 1];
    acc2 += Mc[3 * HID + 2];
    if (valid) {
        const size_t plane = (size_t)p.Hu * p.Wu;
        float* __restrict__ o = p.out + (size_t)b * 3 * plane + (size_t)y * p.Wu + x;
        o[0] = acc0;
        o[plane] = acc1;
        o[2 * plane] = acc2;
    }
}

extern "C" {

int diinn_metasr_decode_hoisted(void* stream, const float* M_dev, const float* packed_dev, float* out_dev,
                                int B, int H, int W, int Hu, int Wu, int y0, int y1) {
    if (!M_dev || !packed_dev || !out_dev) return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if (y0 < 0 || y1 < y0 || y1 > Hu) return DIINN_ERR_INVALID_ARG;
    if (((size_t)M_dev) & 15) return DIINN_ERR_INVALID_ARG;               // 16-byte loads of the M rows
    if ((double)Hu * Wu >= 2.0e9) return DIINN_ERR_TOO_LARGE;
    const long long gx = ((long long)Wu + MH_BLOCK_W - 1) / MH_BLOCK_W;
    const long long gy = ((long long)(y1 - y0) + MH_BLOCK_H - 1) / MH_BLOCK_H;
    if (gy > 65535 || B > 65535) return DIINN_ERR_TOO_LARGE;
    if (y1 == y0) return DIINN_OK;
    MetaHoistParams p;
    p.M = M_dev; p.Wt = packed_dev; p.out = out_dev;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu; p.y0 = y0; p.y1 = y1;
    p.ah = make_meta_axis(H, Hu);
    p.aw = make_meta_axis(W, Wu);
    hipLaunchKernelGGL(metasr_hoisted_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

}  // extern "C"
