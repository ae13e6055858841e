// diinn_enc_training.hip -- the two kernels the RDN dense blocks need under autograd beside the trunk's convolution kernels
// (encoder_training.py: RDBFunction): relu_gate_kernel and conv_wgrad_kernel.  The input gradients of a block run on the forward's own
// kernels (diinn_conv_ksplit / diinn_conv_wino / diinn_conv_wino4_ws with transposed, flipped weights).
#include "diinn_device.h"

// ---------------------------------------------------------------------------------
// relu_gate_kernel: g = y > 0 ? d : 0 over 64 planes per image (rdn.py:15-17 under autograd: the ReLU of a dense layer, whose
// saved output is its own mask).  -0.0, 0.0 and NaN in y close the gate.  Pure streaming: 16-byte accesses where the three
// pointers and batch strides allow, one float per thread otherwise and for the tail.
// ---------------------------------------------------------------------------------
struct ReluGateParams {
    const float* d;
    const float* y;
    float* g;
    long long d_bs, y_bs, g_bs;
    long long n;             // 64 * H * W floats per image
    int vec;                 // 1: the first n / 4 * 4 floats of every image go as f32x4
};

__global__ __launch_bounds__(256) void relu_gate_kernel(const ReluGateParams p) {
    const long long b = blockIdx.y;
    const float* __restrict__ d = p.d + b * p.d_bs;
    const float* __restrict__ y = p.y + b * p.y_bs;
    float* __restrict__ g = p.g + b * p.g_bs;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p.vec) {
        const long long n4 = p.n >> 2;
        if (i < n4) {
            const f32x4 dv = ((const f32x4*)d)[i], yv = ((const f32x4*)y)[i];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = yv[e] > 0.0f ? dv[e] : 0.0f;
            ((f32x4*)g)[i] = o;
        } else if (i - n4 < (p.n & 3)) {                          // the scalar tail
            const long long k = (n4 << 2) + (i - n4);
            g[k] = y[k] > 0.0f ? d[k] : 0.0f;
        }
    } else if (i < p.n) {
        g[i] = y[i] > 0.0f ? d[i] : 0.0f;
    }
}

// ---------------------------------------------------------------------------------
// conv_wgrad_kernel: dW[co][ci][tap] = sum over (b, y, x) of g[b][co][y][x] * x[b][ci][y + ky - 1][x + kx - 1]   (zero padding)
// for 64 output rows -- a GEMM [64 x npix] . [npix x Cin * taps] on the fp32 MFMA whose reduction axis is the pixel axis and whose
// B operand is the NCHW buffer itself read with the tap's shift: the unfold (9 x 576 planes per dense block) is never written.
//
// Workgroup (cb, ks) = 64 input channels x pixel slice ks.  A pixel tile is TW x TH = 32 pixels of one image (32 x 1, 16 x 2 or
// 8 x 4, chosen per map so that ragged tiles waste the least; taps = 1 sees the image as one row of H * W pixels).  Per tile the
// workgroup stages g [64][32] and the x window [64][(TH + 2) x (TW + 2)] (out-of-map positions as zeros) in LDS, then every wave
// = (half of co, half of ci) runs 16 k-steps of 2 pixels x TAPS MFMAs: the A fragment g[co][pixel] is read once per step, the B
// fragment x[ci][pixel + tap shift] once per tap, all at compile-time LDS offsets.  TAPS x 16 accumulator registers per lane.
// The next tile's global loads are issued before the MFMAs of this one and deposited in the other LDS stage after them: one
// barrier per tile.  Row pitches are odd (33, XR * XC + 1), so the 32 rows a fragment read touches fall in 32 banks.
// Slice ks writes part[ks][64][Cin * TAPS + 1]; the extra column holds the row sums of g (the bias gradient; written by the
// workgroups of cb = 0).  A slice without tiles writes zeros.  No atomics: diinn_sum_parts adds the slices in order.
// ---------------------------------------------------------------------------------
struct ConvWgradParams {
    const float* g;          // [B][64][H][W] at g + b * g_bs
    const float* x;          // [B][Cin][H][W] at x + b * x_bs
    float* part;             // [nsplit][64][ldc]
    long long g_bs, x_bs;
    long long ntiles;        // B * tiles_y * tiles_x
    long long tiles_per_split;
    int Cin, H, W, ldc;
    int tiles_x, tiles_y;
};

template <int TAPS, int TW>
__global__ __launch_bounds__(256, 1) void conv_wgrad_kernel(const ConvWgradParams p) {
    constexpr int TH = 32 / TW;
    constexpr int PAD = TAPS == 9 ? 1 : 0;
    constexpr int XR = TH + 2 * PAD, XC = TW + 2 * PAD;
    constexpr int XS = XR * XC + 1;                               // odd row pitch of the x window
    constexpr int GS = 33;                                        // odd row pitch of the g tile
    constexpr int XE = 64 * XR * XC;                              // window elements per tile
    constexpr int XN = (XE + 255) / 256;
    constexpr int STAGE = 64 * XS + 64 * GS;
    __shared__ float lds[2 * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int cb = blockIdx.x, ks = blockIdx.y;
    const int co0 = 32 * (wave & 1), ci0 = 32 * (wave >> 1);
    const long long hw = (long long)p.H * p.W;

    const long long t0 = (long long)ks * p.tiles_per_split;
    long long t1 = t0 + p.tiles_per_split;
    if (t1 > p.ntiles) t1 = p.ntiles;

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    float rs = 0.0f;

    float xv[XN], gv[8];
    auto fetch = [&](long long t) {                               // tile t of the launch -> registers (zeros outside the map)
        const int per_image = p.tiles_x * p.tiles_y;
        const int b = (int)(t / per_image);
        const int rem = (int)(t - (long long)b * per_image);
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
        const int y0 = ty * TH, x0 = tx * TW;
        const float* __restrict__ xb = p.x + (long long)b * p.x_bs + (long long)cb * 64 * hw;
        const float* __restrict__ gb = p.g + (long long)b * p.g_bs;
#pragma unroll
        for (int i = 0; i < XN; ++i) {
            const int e = i * 256 + tid;
            const int ci = e / (XR * XC), w = e - ci * (XR * XC);
            const int r = w / XC, c = w - r * XC;
            const int yy = y0 + r - PAD, xx = x0 + c - PAD;
            const bool in = e < XE && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
            xv[i] = in ? xb[(long long)ci * hw + (long long)yy * p.W + xx] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = i * 256 + tid;
            const int co = e >> 5, px = e & 31;
            const int yy = y0 + px / TW, xx = x0 + px % TW;
            const bool in = yy < p.H && xx < p.W;
            gv[i] = in ? gb[(long long)co * hw + (long long)yy * p.W + xx] : 0.0f;
        }
    };
    auto deposit = [&](int st) {
        float* __restrict__ xs = lds + st * STAGE;
        float* __restrict__ gs = xs + 64 * XS;
#pragma unroll
        for (int i = 0; i < XN; ++i) {
            const int e = i * 256 + tid;
            const int ci = e / (XR * XC), w = e - ci * (XR * XC);
            if (e < XE) xs[ci * XS + w] = xv[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = i * 256 + tid;
            gs[(e >> 5) * GS + (e & 31)] = gv[i];
        }
    };

    if (t0 < t1) {
        fetch(t0);
        deposit(0);
    }
    __syncthreads();
    int st = 0;
    for (long long t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;
        if (more) fetch(t + 1);
        const float* __restrict__ xs = lds + st * STAGE + (ci0 + j) * XS + h;
        const float* __restrict__ gs = lds + st * STAGE + 64 * XS + (co0 + j) * GS + h;
#pragma unroll
        for (int s = 0; s < 16; ++s) {                            // pixels 2 s + h of the tile: row (2 s) / TW, column (2 s) % TW + h
            const float a = gs[2 * s];
            const int py = (2 * s) / TW, px = (2 * s) % TW;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int ky = TAPS == 9 ? tap / 3 : 0, kx = TAPS == 9 ? tap % 3 : 0;
                const float bv = xs[(py + ky) * XC + px + kx];
                acc[tap] = MFMA32(a, bv, acc[tap]);
            }
            rs += a;
        }
        if (more) deposit(st ^ 1);
        __syncthreads();
        st ^= 1;
    }

    float* __restrict__ dst = p.part + (size_t)ks * 64 * p.ldc;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            dst[(size_t)co * p.ldc + (size_t)(cb * 64 + ci0 + j) * TAPS + tap] = acc[tap][r];
        }
    if (cb == 0 && ci0 == 0) {                                    // wave-uniform: the row sums of g, once per slice
        const float v = rs + __shfl_xor(rs, 32);
        if (h == 0) dst[(size_t)(co0 + j) * p.ldc + (size_t)p.Cin * TAPS] = v;
    }
}

template <int TAPS, int TW>
static void launch_wgrad(hipStream_t stream, const ConvWgradParams& p, int nsplit) {
    hipLaunchKernelGGL((conv_wgrad_kernel<TAPS, TW>), dim3((unsigned)(p.Cin / 64), (unsigned)nsplit), dim3(256), 0, stream, p);
}

extern "C" {

int diinn_relu_gate(void* stream, const float* d_dev, long long d_batch_stride, const float* y_dev, long long y_batch_stride,
                    float* g_dev, long long g_batch_stride, int B, int H, int W) {
    if (!d_dev || !y_dev || !g_dev) return DIINN_ERR_INVALID_ARG;
    const int st = check_dims(B, H, W);
    if (st) return st;
    const long long n = 64LL * H * W;
    if (d_batch_stride < 0 || y_batch_stride < 0 || g_batch_stride < 0) return DIINN_ERR_INVALID_ARG;
    if (B > 1 && (d_batch_stride < n || y_batch_stride < n || g_batch_stride < n)) return DIINN_ERR_INVALID_ARG;
    if ((((size_t)d_dev) | ((size_t)y_dev) | ((size_t)g_dev)) & 3) return DIINN_ERR_INVALID_ARG;
    ReluGateParams p{d_dev, y_dev, g_dev, d_batch_stride, y_batch_stride, g_batch_stride, n, 0};
    p.vec = !((((size_t)d_dev) | ((size_t)y_dev) | ((size_t)g_dev)) & 15) &&
            !((d_batch_stride | y_batch_stride | g_batch_stride) & 3);
    const long long threads = p.vec ? (n >> 2) + (n & 3) : n;
    const long long blocks = (threads + 255) / 256;
    if (blocks > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    hipLaunchKernelGGL(relu_gate_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

int diinn_conv_wgrad(void* stream, const float* g_dev, long long g_batch_stride, const float* x_dev, long long x_batch_stride,
                     int Cin, int taps, float* part_dev, int nsplit, int B, int H, int W) {
    if (!g_dev || !x_dev || !part_dev || nsplit <= 0) return DIINN_ERR_INVALID_ARG;
    const int st = check_dims(B, H, W);
    if (st) return st;
    if (taps != 9 && taps != 1) return DIINN_ERR_UNSUPPORTED;
    if (Cin <= 0 || Cin % 64 || Cin > 576) return DIINN_ERR_UNSUPPORTED;
    if (g_batch_stride < 0 || x_batch_stride < 0) return DIINN_ERR_INVALID_ARG;
    if ((((size_t)g_dev) | ((size_t)x_dev) | ((size_t)part_dev)) & 3) return DIINN_ERR_INVALID_ARG;
    if (nsplit > 65535) return DIINN_ERR_TOO_LARGE;
    if ((long long)H * W > 2147483000LL / 64) return DIINN_ERR_TOO_LARGE;    // tile arithmetic inside one image is 32-bit
    ConvWgradParams p;
    p.g = g_dev; p.x = x_dev; p.part = part_dev; p.g_bs = g_batch_stride; p.x_bs = x_batch_stride;
    p.Cin = Cin; p.ldc = Cin * taps + 1;
    int tw = 32;
    if (taps == 1) {                                             // no neighbours: the image is one row of H * W pixels
        p.H = 1; p.W = H * W;
    } else {
        p.H = H; p.W = W;
        long long best = -1;
        for (int c = 32; c >= 8; c /= 2) {                       // the tile shape with the fewest tiles (ties: the widest)
            const long long n = (long long)((W + c - 1) / c) * ((H + 32 / c - 1) / (32 / c));
            if (best < 0 || n < best) { best = n; tw = c; }
        }
    }
    p.tiles_x = (p.W + tw - 1) / tw;
    p.tiles_y = (p.H + 32 / tw - 1) / (32 / tw);
    if ((long long)p.tiles_x * p.tiles_y > 2147483000LL) return DIINN_ERR_TOO_LARGE;
    p.ntiles = (long long)B * p.tiles_x * p.tiles_y;
    p.tiles_per_split = (p.ntiles + nsplit - 1) / nsplit;
    const hipStream_t s = (hipStream_t)stream;
    if (taps == 1) launch_wgrad<1, 32>(s, p, nsplit);
    else if (tw == 32) launch_wgrad<9, 32>(s, p, nsplit);
    else if (tw == 16) launch_wgrad<9, 16>(s, p, nsplit);
    else launch_wgrad<9, 8>(s, p, nsplit);
    return hip_status(hipGetLastError());
}

}  // extern "C"
