// diinn_mode4_training.hip -- training forward of decoder mode 4: the 27 tap values of the 3x3 head from the SAVED planes
// (part of libdiinn_hip.so; shared definitions in diinn_device.h, layout in diinn_layout.h)
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// head3x3_taps_from_planes_kernel (training forward, decoder mode 4; reference: last_layer of diinn.py:89-90,146 under autograd)
//
// Mode 4 is mode 3 up to q_3 = k_3 * sin(s_3), and the mode-3 training forward (decode_kernel<SAVE>) leaves k_3 and s_3 as group 3
// of its tiled planes [T][512][32].  This kernel reads that group (2 KiB per HR pixel), forms q_3 with the reduction the backward
// pass uses for its Q planes (dsincos, diinn_device.h), and writes T[pix][r] = H[r] . q_3 (r = 3 k + c, 27 values) in
// the tap-buffer layout of the inference path, [B][Hu][Wu][TAP_STRIDE] = [npix][28] (float 27 zero): head3x3_reflect_kernel gathers
// nine of them per output, unchanged.
//
// The product is a [32 x 256] . [256 x 32 pixels] GEMM per plane tile (head rows 27..31 zero) on the fp32 MFMA, one wave per tile:
//   A operand: the head rows, held in 128 registers for the wave's lifetime (a wave walks tiles): k-step s of lane (j, h) is
//              H[row j][channel s + 128 h] -- the sum over channels does not care which two meet in a k-step;
//   B operand: q_3[channel s + 128 h][pixel j], formed in registers from the two loads (k, s) of that plane element -- a wave
//              instruction reads two full 128-byte rows; the loads of the next 16 k-steps go out in front of the current 16's MFMAs;
//   C        : lane (j, h) ends with taps (r & 3) + 8 (r >> 2) + 4 h of pixel j: four (h = 1: three) 16-byte stores into the pixel's
//              112-byte record.
// No LDS, no barrier: the kernel is bound by the 2 KiB per pixel it reads (128 MFMAs per 64 KiB tile).  A fixed order of addition.
// Ragged last tile: a lane past the last pixel loads nothing (the planes' padding was never written) and stores nothing.
// Validity: the body image's word must be DIINN_PACKED_MAGIC or DIINN_PACKED_MAGIC_WPU (a training image), the head image's
// DIINN_HEAD3X3_MAGIC; otherwise every tap value is NaN.
// ---------------------------------------------------------------------------------
struct TapsFromPlanesParams {
    const float* acts3;      // group 3 of the training forward's planes: [ntiles][512][32], rows 0..255 k_3, 256..511 s_3
    const float* Wt;         // body image (validity word only)
    const float* head3;      // head image [27][256], bias, validity word
    float* taps;             // [npix][TAP_STRIDE]
    long long npix, ntiles;
};

__global__ __launch_bounds__(256) void head3x3_taps_from_planes_kernel(const TapsFromPlanesParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const unsigned bw = __builtin_bit_cast(unsigned, p.Wt[OFF_BL + 3]);
    const unsigned nanm = ((bw == DIINN_PACKED_MAGIC || bw == DIINN_PACKED_MAGIC_WPU) &&
                           __builtin_bit_cast(unsigned, p.head3[HEAD3_BIAS + 3]) == DIINN_HEAD3X3_MAGIC) ? 0u : 0x7fc00000u;
    float hw[128];                                               // A operand: H[j][128 h + s], rows 27..31 zero
    {
        const f32x4* __restrict__ hr = (const f32x4*)(p.head3 + (size_t)(j < TAPS ? j : 0) * HID + 128 * h);
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const f32x4 v = hr[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) hw[4 * i + e] = j < TAPS ? v[e] : 0.0f;
        }
    }
    constexpr int CH = 16;                                       // k-steps per load group
    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < p.ntiles; tile += (long long)gridDim.x * 4) {
        const long long pix = tile * PLANE_TILE + j;
        const bool valid = pix < p.npix;
        const float* __restrict__ a = p.acts3 + (size_t)tile * ACT_ROWS * PLANE_TILE + (size_t)(128 * h) * PLANE_TILE + j;
        float kv[2][CH], sv[2][CH];
        auto load_group = [&](int buf, int g) {
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const int c = CH * g + e;
                kv[buf][e] = valid ? __builtin_nontemporal_load(a + (size_t)c * PLANE_TILE) : 0.0f;
                sv[buf][e] = valid ? __builtin_nontemporal_load(a + (size_t)(HID + c) * PLANE_TILE) : 0.0f;
            }
        };
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        load_group(0, 0);
#pragma unroll
        for (int g = 0; g < 128 / CH; ++g) {
            if (g + 1 < 128 / CH) load_group((g + 1) & 1, g + 1);
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                float sn, cs;
                dsincos(sv[g & 1][e], sn, cs);
                acc = MFMA32(hw[CH * g + e], kv[g & 1][e] * sn, acc);
            }
        }
        if (valid) {
            float* __restrict__ t = p.taps + (size_t)pix * TAP_STRIDE + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (8 * g + 4 * h < TAP_STRIDE) {                 // (h = 1, g = 3: taps 28..31 do not exist)
                    // (h = 0, g = 3: taps 24, 25, 26 and the pad float, which stays an exact zero -- head row 27 is zero)
                    const float last = (g == 3) ? acc[4 * g + 3] : or_bits(acc[4 * g + 3], nanm);
                    *(f32x4*)(t + 8 * g) = f32x4{or_bits(acc[4 * g], nanm), or_bits(acc[4 * g + 1], nanm), or_bits(acc[4 * g + 2], nanm), last};
                }
            }
        }
    }
}

// diinn_decode.hip: head3x3_reflect_kernel over the whole image, for a tap buffer whose producer has checked the body image
__attribute__((visibility("hidden")))
int launch_head3x3_whole(void* stream, const float* taps_dev, const float* head_dev, float* out_dev, int B, int Hu, int Wu);

extern "C" {

int diinn_head3x3_from_planes(void* stream, const float* acts_dev, const float* packed_dev, const float* head_dev,
                              float* taps_dev, float* out_dev, int B, int Hu, int Wu) {
    if (!acts_dev || !packed_dev || !head_dev || !taps_dev || !out_dev) return DIINN_ERR_INVALID_ARG;
    if (B <= 0 || Hu < 2 || Wu < 2) return DIINN_ERR_INVALID_ARG;
    const long long npix = (long long)B * Hu * Wu;
    const int stp = check_npix(npix);
    if (stp) return stp;
    if (B > 65535 || (Hu + 3) / 4 > 65535) return DIINN_ERR_TOO_LARGE;
    if ((((size_t)acts_dev) | ((size_t)head_dev) | ((size_t)taps_dev)) & 15) return DIINN_ERR_INVALID_ARG;   // 16-byte loads and stores
    TapsFromPlanesParams p;
    p.npix = npix; p.ntiles = (npix + PLANE_TILE - 1) / PLANE_TILE;
    p.acts3 = acts_dev + (size_t)3 * p.ntiles * ACT_ROWS * PLANE_TILE;
    p.Wt = packed_dev; p.head3 = head_dev; p.taps = taps_dev;
    // a wave owns a tile at a time; two workgroups per compute unit walk the tiles (the head rows are fetched once per wave)
    const long long cap = 2LL * device_cus(), need = (p.ntiles + 3) / 4;
    const unsigned blocks = (unsigned)(need < cap ? need : cap);
    hipLaunchKernelGGL(head3x3_taps_from_planes_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    const int st = hip_status(hipGetLastError());
    if (st) return st;
    return launch_head3x3_whole(stream, taps_dev, head_dev, out_dev, B, Hu, Wu);
}

}  // extern "C"
