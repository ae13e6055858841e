// diinn_initq_split_training.hip -- decoder init_q=True, mode 3, under autograd in split-bf16 arithmetic (behind
// ImplicitDecoder.hip_autograd_initq_split_bf16): the device packer of the init_q split training image and initq_bwd_kernel's two
// transposed per-pixel GEMMs on v_mfma_f32_32x32x16_bf16.
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h.  The forward of the same switch is
// initq_planes_x3_kernel<SIN | INITQ_X3_RAD> in diinn_initq_x3.hip and decode_bf16x3_kernel<SIN | X3_INITQ | X3_SAVE> in
// diinn_bf16x3.hip; the chain is bwd_layer_x3_kernel in diinn_split_training.hip, unchanged.)
#include "diinn_device.h"

__device__ __forceinline__ static void split2_bf16(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);               // exact difference: v and hi share sign and exponent range
}

// ---------------------------------------------------------------------------------
// initq_split_train_pack_kernel: section WP of the (gathered) body image and the Q0W part of the init_q training image -> the
// init_q split training image (diinn_layout.h).  A thread owns one lane of one pair of pieces: its eight weights are eight floats
// of the source (iqs_source: the layout's one statement, shared with the host twin diinn_pack_initq_split_train_host; the tests
// compare the two bit for bit), written as one 16-byte hi and one 16-byte lo run.  hi = bf16(w), lo = bf16(w - hi), round to
// nearest even.  Thread 0 writes the validity word.  6 MiB written: runs once per weight version.
// ---------------------------------------------------------------------------------
constexpr int IQS_PACK_THREADS = IQS_PAIRS * 64;                 // 194,560

__global__ __launch_bounds__(256) void initq_split_train_pack_kernel(const float* __restrict__ body, const float* __restrict__ train,
                                                                     float* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= IQS_PACK_THREADS) return;
    const int lane = t & 63, pair = t >> 6;
    bf16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int img;
        const size_t at = iqs_source(pair, lane, j, img);
        const float v = img < 0 ? 0.0f : (img ? train : body)[at];
        __bf16 vh, vl;
        split2_bf16(v, vh, vl);
        hi[j] = vh; lo[j] = vl;
    }
    bf16x8* __restrict__ dst = (bf16x8*)(out + iqs_pair_offset(pair)) + lane;
    dst[0] = hi;
    dst[64] = lo;
    if (t == 0) *(u32x4*)(out + IQS_OFF_WORD) = u32x4{DIINN_INITQ_SPLIT_TRAIN_MAGIC, 0u, 0u, 0u};
}

// ---------------------------------------------------------------------------------
// initq_bwd_x3_kernel: initq_bwd_kernel (diinn_initq_training.hip) with its two reductions on the bf16 matrix cores,
//     D1 [640 x pixels] = WxT [640 x 1024] . (g_a,0 ; .. ; g_a,3)      D2 = Q0T [640 x 256] . g_s,0
// every operand carried as hi + lo (hi = bf16(v), lo = bf16(v - hi)) and a product formed as w_lo.g_hi + w_hi.g_lo + w_hi.g_hi with
// fp32 accumulation, the three terms of a k-step added to the accumulator in that order (the forward's rule).
// Workgroup = 4 waves = 64 pixels = two plane tiles = two N-tiles; a wave owns 5 of the 20 M-tiles (rows 576..639 zero padding)
// against both N-tiles: 160 accumulator registers per reduction.
//   * B operand.  The reduction runs in five CHUNKS of 256 rows (the g_s rows of G_0 first, then the g_a rows of G_0..G_3).  A
//     chunk of both tiles is fetched ONCE per workgroup -- 64 dwords per thread, a row segment of a tile is one 128-byte line --
//     split to hi/lo on the way into LDS and stored as the MFMA's B fragments [k-step 16][hi, lo][N-tile 2][lane 64] of 16 bytes
//     (64 KiB; fragment element j of k-step ks is row 16 ks + 8 (lane >> 5) + j of the chunk at pixel lane & 31), which all four
//     waves read back with four conflict-free ds_read_b128 per k-step.  Two such buffers: the next chunk is staged under the
//     current chunk's MFMAs, a thread's eight fragments one per pair of k-steps (eight loads in the even k-step, the split and the
//     two LDS stores in the odd one); one barrier per chunk.
//   * A operand.  Sections WXT / Q0T of the init_q split training image, per wave [chunk][ks][M-tile 5][hi, lo]: the ten 1 KiB pieces
//     of a k-step are contiguous (one scalar offset, immediate offsets) and arrive through a register ring two k-steps deep; they
//     feed 30 MFMAs.
//   * What the k = 16 step settles (the question initq_bwd_kernel left): G IS STAGED ONCE.  All five M-tiles of a wave run in one
//     pass over each chunk.  D1 and D2 together are still 320 accumulators -- the k = 16 step changes the operand's depth, not the
//     tile's size -- so they are not held together: D2 (one chunk) is reduced FIRST and parked as fp32 in dA's own storage (each
//     element written and read back by the same lane: no other thread touches it, nothing is atomic), then D1 (four chunks) runs in
//     the same registers and the epilogue fetches t back.  That costs 2,304 bytes per pixel each way against the 5,120 bytes per
//     pixel of a second staging pass, and the weight stream is read once.
//   * Epilogue: fp32, initq_bwd_kernel's term for term -- a by the forward's operation order (fma(Fr, ratio, bF), then rel_w, then
//     rel_h), sin a and cos a by dsincos's reduction, X by the forward's clamped load and select, U = dx' E, dA = (dx' X + t) cos a,
//     x' = E X and E (640 rows, the padding rows written as zeros).  F comes from the init_q training image, in radians.  The
//     accumulators of an N-tile pass through the wave's own 20 KiB of the (then idle) staging buffers, each lane re-reading what it
//     wrote, so that the epilogue is a LOOP over the M-tiles' rows: unrolled over all 160 elements per lane it kept 200 addresses
//     live and spilled.
// A pixel is one column of the GEMM: the columns of a ragged last tile's padding and of a tile past the end are fetched as zeros
// (an offset outside the descriptor), meet no other column and are not stored.  No atomics, no scratch, fixed summation order, one
// workgroup per CU.
// What bounds it: profiles/initq_x3_train_times.txt.
// ---------------------------------------------------------------------------------
struct InitqBwdX3Params {
    const float* feat;       // [B,64,H,W]
    const float* G;          // tiled [4][ntiles][512][32]
    const float* img;        // the init_q training image (F, in radians)
    const float* iqs;        // the init_q split training image (WXT, Q0T)
    float* U;                // tiled [ntiles][576][32]   dx' * E
    float* dA;               // tiled [ntiles][576][32]   d loss / d a  (holds t between the two reductions)
    float* XP;               // tiled [ntiles][640][32]   x' (rows 576.. zero)
    float* E;                // tiled [ntiles][640][32]   E  (rows 576.. zero)
    long long npix, ntiles;
    int B, H, W, Hu, Wu;
    float ratio;
    Axis ah, aw;
};

constexpr int IBX_KS_BYTES = (int)(IQS_KSTEP * sizeof(float));   // a wave's k-step of weights: 10 KiB
constexpr int IBX_RING = 2;                                      // weight ring depth in k-steps

// t on its way to dA and back: a plain store (no streaming hint: the same lane reads the element back).  The value travels as a
// float argument, as in st_act.
__device__ __forceinline__ static void st_park(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc, (int)voff, (int)soff, 0);
}

typedef float __attribute__((may_alias)) f32_lds;
typedef f32x4 __attribute__((may_alias)) f32x4_ldsv;

__global__ __launch_bounds__(256, 1) void initq_bwd_x3_kernel(const InitqBwdX3Params p) {
    __shared__ __attribute__((aligned(16))) bf16x8 bfrag[2][16][2][2][64];   // [buffer][k-step][hi, lo][N-tile][lane] = 2 x 64 KiB
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const long long tile0 = (long long)blockIdx.x * 2;
    const size_t agroup = (size_t)p.ntiles * ACT_ROWS * PLANE_TILE;
    // an image without its validity word answers NaN in every output
    const bool img_ok = __builtin_bit_cast(unsigned, p.iqs[IQS_OFF_WORD]) == DIINN_INITQ_SPLIT_TRAIN_MAGIC &&
                        __builtin_bit_cast(unsigned, p.img[IQ_OFF_BQ0 + HID]) == DIINN_INITQ_TRAIN_MAGIC;
    const unsigned nanm = img_ok ? 0u : 0x7fc00000u;

    // per N-tile: is this lane's pixel one of the image's?  The offsets of lanes that are not lie outside every descriptor: their
    // loads return zeros, their stores are dropped.  (Recomputed where used: as two-element arrays, indexed inside loops that are
    // unrolled late, they were moved to LDS.)
    auto lane_valid = [&](const int nt) { return tile0 + nt < p.ntiles && (tile0 + nt) * PLANE_TILE + j < p.npix; };
    auto voff_of = [&](const int nt) { return lane_valid(nt) ? 4u * j + 4u * h * PLANE_ROW_BYTES : 0xFFFFFFF0u; };   // epilogue: pixel j in the row of lane half h x 4
    auto goff_of = [&](const int nt) { return lane_valid(nt) ? 4u * j + 8u * h * PLANE_ROW_BYTES : 0xFFFFFFF0u; };   // staging:  pixel j in the row of lane half h x 8

    // ---- staging.  Chunk c = 0..3: the g_a rows (0..255) of G_c; chunk 4: the g_s rows (256..511) of G_0.  Thread (wave, lane)
    // owns the fragments (ks, nt) = ((wave + 4 i) >> 1, (wave + 4 i) & 1), i = 0..7, of its lane in every chunk.
    float sg[8];
    auto fetch_frag = [&](const int c, const int i) {
        const float* grp = p.G + (size_t)(c < 4 ? c : 0) * agroup;
        const unsigned rowbase = c < 4 ? 0u : (unsigned)HID;
        const int f = wave + 4 * i;                              // wave-uniform
        const int ks = f >> 1, nt = f & 1;
        const long long tile = tile0 + nt;
        const __amdgpu_buffer_rsrc_t rs = tile_rsrc(grp, tile < p.ntiles ? tile : 0, ACT_ROWS);
        const unsigned so = (rowbase + 16u * ks) * PLANE_ROW_BYTES;
        const unsigned vo = goff_of(nt);
#pragma unroll
        for (int e = 0; e < 8; ++e) sg[e] = ld_act(rs, vo, so + e * PLANE_ROW_BYTES);
    };
    auto store_frag = [&](const int buf, const int i) {
        const int f = wave + 4 * i;
        const int ks = f >> 1, nt = f & 1;
        bf16x8 gh, gl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            __bf16 vh, vl;
            split2_bf16(sg[e], vh, vl);
            gh[e] = vh; gl[e] = vl;
        }
        bfrag[buf][ks][0][nt][lane] = gh;
        bfrag[buf][ks][1][nt][lane] = gl;
    };

    // ---- the weight stream of this wave: byte offset of chunk c's first k-step
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.iqs, 0, (int)(IQS_FLOATS * sizeof(float)), 0x00020000);
    const int lane_off = lane * 16;
    auto chunk_off = [&](const int c) -> int {
        return c < 4 ? (int)(IQS_OFF_WXT * sizeof(float)) + (wave * 4 + c) * 16 * IBX_KS_BYTES
                     : (int)(IQS_OFF_Q0T * sizeof(float)) + wave * 16 * IBX_KS_BYTES;
    };
    f32x4 rw[IBX_RING][2 * IQT_MT];                              // [slot][M-tile 0 hi, lo, M-tile 1 hi, lo, ...]
    auto ld_kstep = [&](const int slot, const int soff) {
#pragma unroll
        for (int q = 0; q < 2 * IQT_MT; ++q) rw[slot][q] = ld_piece(wrs, lane_off + q * PIECE_BYTES, soff);
    };

    f32x16 acc[IQT_MT][2];                                       // [M-tile][N-tile]
    auto zero_acc = [&]() {
#pragma unroll
        for (int mt = 0; mt < IQT_MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.0f;
    };
    // one chunk from buffer `buf`: 16 k-steps x 30 MFMAs.  Chunk `cn` follows (cn < 0: nothing does): its fragments are staged
    // into the other buffer and the weight ring runs on into it.
    auto run_chunk = [&](const int c, const int cn, const int buf) {
        const int wp = chunk_off(c), wn = cn >= 0 ? chunk_off(cn) : 0;
        int off = lane;
        asm volatile("" : "+v"(off));                            // (the fragment reads stay inside the chunk loop)
        const bf16x8* bm = &bfrag[buf][0][0][0][0] + off;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            if (cn >= 0 && (ks & 1) == 0) fetch_frag(cn, ks >> 1);
            const bf16x8 gh[2] = {bm[((2 * ks + 0) * 2 + 0) * 64], bm[((2 * ks + 0) * 2 + 1) * 64]};
            const bf16x8 gl[2] = {bm[((2 * ks + 1) * 2 + 0) * 64], bm[((2 * ks + 1) * 2 + 1) * 64]};
            // the two small products first, the leading one last
#pragma unroll
            for (int mt = 0; mt < IQT_MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = MFMA_BF16(__builtin_bit_cast(bf16x8, rw[ks % IBX_RING][2 * mt + 1]), gh[nt], acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < IQT_MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = MFMA_BF16(__builtin_bit_cast(bf16x8, rw[ks % IBX_RING][2 * mt + 0]), gl[nt], acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < IQT_MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = MFMA_BF16(__builtin_bit_cast(bf16x8, rw[ks % IBX_RING][2 * mt + 0]), gh[nt], acc[mt][nt]);
            if (ks + IBX_RING < 16) ld_kstep(ks % IBX_RING, wp + (ks + IBX_RING) * IBX_KS_BYTES);
            else if (cn >= 0) ld_kstep(ks % IBX_RING, wn + (ks + IBX_RING - 16) * IBX_KS_BYTES);
            if (cn >= 0 && (ks & 1) == 1) store_frag(buf ^ 1, ks >> 1);
            __builtin_amdgcn_sched_barrier(0);                   // the region ends at the k-step (the ring loads stay ahead)
        }
    };
    static_assert(16 % IBX_RING == 0, "ring index must be static");

    // ---- reduction 1: t = Q0T . g_s,0 (chunk 4, buffer 0), parked in dA
#pragma unroll
    for (int d = 0; d < IBX_RING; ++d) ld_kstep(d, chunk_off(4) + d * IBX_KS_BYTES);
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
        fetch_frag(4, i);
        store_frag(0, i);
    }
    zero_acc();
    __syncthreads();
    run_chunk(4, 0, 0);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const long long tile = tile0 + nt;
        if (tile >= p.ntiles) continue;                          // wave-uniform
        const __amdgpu_buffer_rsrc_t rA = tile_rsrc(p.dA, tile, UNF);
#pragma unroll
        for (int mt = 0; mt < IQT_MT; ++mt) {
            const int mtg = IQT_MT * wave + mt;                  // wave-uniform
            if (mtg >= UNF / 32) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                st_park(rA, voff_of(nt), (unsigned)(32 * mtg + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES, acc[mt][nt][r]);
        }
    }
    __syncthreads();                                             // chunk 0 is staged; everybody is done with chunk 4

    // ---- reduction 2: dx' = WxT . (g_a,0 ; .. ; g_a,3) (chunks 0..3, buffers 1, 0, 1, 0)
    zero_acc();
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        run_chunk(c, c < 3 ? c + 1 : -1, (c + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue (initq_bwd_kernel's, with t fetched back from dA).  Every wave is behind the last barrier: the staging buffers
    // are idle, and this wave's 20 KiB of them take the accumulators of one N-tile as [M-tile 5][r >> 2][lane][r & 3].
    const float* __restrict__ F = p.img + IQ_OFF_F;
    const int hw = p.Hu * p.Wu;
    f32x4_ldsv* const accv = (f32x4_ldsv*)&bfrag[0][0][0][0][0] + wave * (IQT_MT * 4 * 64) + lane;
    const f32_lds* const accl = (const f32_lds*)accv;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const long long tile = tile0 + nt;
        if (tile >= p.ntiles) continue;                          // wave-uniform
#pragma unroll
        for (int mt = 0; mt < IQT_MT; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x16& a = acc[mt][nt];
                accv[(mt * 4 + g) * 64] = f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
            }
        const long long pix = tile * PLANE_TILE + j;
        const long long pc = lane_valid(nt) ? pix : p.npix - 1;       // lanes past the end compute on the last pixel and store nothing
        const int b = (int)(pc / hw);
        const int rem = (int)(pc - (long long)b * hw);
        const int y = rem / p.Wu, x = rem - y * p.Wu;
        int iy, ix;
        float relh, relw;
        axis_eval(p.ah, y, iy, relh);
        axis_eval(p.aw, x, ix, relw);
        const float* __restrict__ fb = p.feat + (size_t)b * C_IN * p.H * p.W;
        const unsigned vo = voff_of(nt);
        const __amdgpu_buffer_rsrc_t rU = tile_rsrc(p.U, tile, UNF), rA = tile_rsrc(p.dA, tile, UNF);
        const __amdgpu_buffer_rsrc_t rX = tile_rsrc(p.XP, tile, IQT_ROWS), rE = tile_rsrc(p.E, tile, IQT_ROWS);
#pragma unroll 1
        for (int mt = 0; mt < IQT_MT; ++mt) {
            const int mtg = IQT_MT * wave + mt;                  // wave-uniform
            if (mtg >= UNF / 32) {                               // the padding rows 576..639 of x' and E
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned so = (unsigned)(32 * mtg + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES;
                    st_act(rX, vo, so, 0.0f);
                    st_act(rE, vo, so, 0.0f);
                }
                continue;
            }
#pragma unroll 1
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n0 = 32 * mtg + e + 8 * g;         // the row of lane-half 0 (wave-uniform); half 1: + 4
                    const int n = n0 + 4 * h;
                    const unsigned so = (unsigned)n0 * PLANE_ROW_BYTES;
                    const float tq = ld_act(rA, vo, so);
                    float a = __builtin_fmaf(F[2 * UNF + n], p.ratio, F[3 * UNF + n]);
                    a = __builtin_fmaf(F[1 * UNF + n], relw, a);
                    a = __builtin_fmaf(F[0 * UNF + n], relh, a);
                    float sn, cs;
                    dsincos(a, sn, cs);
                    const int c = n / 9, tap = n - 9 * c;
                    const int ky = tap / 3, kx = tap - 3 * ky;
                    const int yy = iy + ky - 1, xx = ix + kx - 1;
                    const bool ok = (yy >= 0) && (yy < p.H) && (xx >= 0) && (xx < p.W);
                    const int yc = yy < 0 ? 0 : (yy >= p.H ? p.H - 1 : yy);
                    const int xc = xx < 0 ? 0 : (xx >= p.W ? p.W - 1 : xx);
                    const float v = fb[((size_t)c * p.H + yc) * p.W + xc];
                    const float X = ok ? v : 0.0f;
                    const float dx = or_bits(accl[((mt * 4 + g) * 64) * 4 + e], nanm);
                    const float de = __builtin_fmaf(dx, X, tq);
                    st_act(rU, vo, so, dx * sn);
                    st_act(rA, vo, so, de * cs);
                    st_act(rX, vo, so, or_bits(sn * X, nanm));
                    st_act(rE, vo, so, or_bits(sn, nanm));
                }
            }
        }
    }
}

extern "C" {

int diinn_pack_initq_split_train(void* stream, const float* packed_dev, const float* train_image_dev, float* initq_split_dev) {
    if (!packed_dev || !train_image_dev || !initq_split_dev) return DIINN_ERR_INVALID_ARG;
    if ((((size_t)packed_dev) | ((size_t)train_image_dev) | ((size_t)initq_split_dev)) & 15) return DIINN_ERR_INVALID_ARG;   // 16-byte stores
    hipLaunchKernelGGL(initq_split_train_pack_kernel, dim3(IQS_PACK_THREADS / 256), dim3(256), 0, (hipStream_t)stream, packed_dev,
                       train_image_dev, initq_split_dev);
    return hip_status(hipGetLastError());
}

int diinn_initq_backward_x3(void* stream, const float* feat_dev, const float* G_dev, const float* train_image_dev,
                            const float* initq_split_dev, float* U_dev, float* dA_dev, float* XP_dev, float* E_dev,
                            int B, int H, int W, int Hu, int Wu) {
    if (!feat_dev || !G_dev || !train_image_dev || !initq_split_dev || !U_dev || !dA_dev || !XP_dev || !E_dev) return DIINN_ERR_INVALID_ARG;
    int st = check_dims(B, H, W);
    if (st) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if ((double)Hu * Wu >= 2.0e9) return DIINN_ERR_TOO_LARGE;
    const long long npix = (long long)B * Hu * Wu;
    st = check_npix(npix);
    if (st) return st;
    // 16-byte weight pieces
    if ((((size_t)train_image_dev) | ((size_t)initq_split_dev)) & 15) return DIINN_ERR_INVALID_ARG;
    InitqBwdX3Params p;
    p.feat = feat_dev; p.G = G_dev; p.img = train_image_dev; p.iqs = initq_split_dev;
    p.U = U_dev; p.dA = dA_dev; p.XP = XP_dev; p.E = E_dev;
    p.npix = npix; p.ntiles = (npix + PLANE_TILE - 1) / PLANE_TILE;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu;
    p.ratio = (float)(((double)H * (double)W) / ((double)Hu * (double)Wu));
    const int small = diinn_uses_small_output_kernel(Hu, Wu);
    p.ah = make_axis(H, Hu, small);
    p.aw = make_axis(W, Wu, small);
    if ((p.ntiles + 1) / 2 > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    hipLaunchKernelGGL(initq_bwd_x3_kernel, dim3((unsigned)((p.ntiles + 1) / 2)), dim3(256), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

}  // extern "C"
