// diinn_decode.hip -- gfx950 (MI355X, CDNA4): the fp32 decode kernel of the DIINN implicit decoder and the
// decode entry points of the C ABI (include/diinn_hip.h).  Sibling translation units: see diinn_device.h.
//
// Reference path replaced: ImplicitDecoder.forward, mode 3
//   /root/reference/src/models/components/diinn.py:163-173 (+ :94-110, :132-139, :149-160)
//
// Kernels (DESIGN.md has the derivation, the roofline and the measurements of each):
//   precompute_P_kernel : per LR cell, P_i = Wx_i . unfold3x3(feat) + bK_i, i=0..3
//                         (implicit-im2col GEMM 576 -> 1024 on v_mfma_f32_32x32x2_f32,
//                         feature halo tile in LDS); precompute_P_bf16_kernel: bf16 operands
//   decode_kernel       : per HR pixel, the dual-branch MLP.  One wave owns 32 pixels
//                         and keeps their 256-channel activation in registers for the
//                         whole network: the accumulator layout of one layer IS the
//                         B-operand layout of the next (diinn_layout.h), so activations
//                         never touch LDS or HBM.  Weights stream from the packed image.
//                         <KPART=false>: decoder modes 1/2 (with cell_chain_kernel);
//                         <SAVE>: training forward, also writes k_i, s_i as tiled planes (with KPART=false: the modes-1/2
//                         training forward, k_i of the pixel's cell replicated per pixel);
//                         <HEAD3>: decoder mode 4, the head is the 27 per-pixel tap values of the 3x3 conv
//   head3x3_reflect_kernel : decoder mode 4, the reflect-padded 9-point gather over the tap buffer
//   cell_chain_kernel, pixel_chain_kernel : decoder modes 1/2, the modulation chain per LR cell / (init_q=True) per HR pixel
//   decode_bf16_kernel, decode_bf16x2_kernel : bf16 operands in layers 1..3 (optional paths)
//   bwd_layer_kernel (+ bwd_head_kernel), plane_gemm_lds_kernel, plane_rowdot_kernel, cell_sum_kernel :
//                         backward pass of the decoder (training)
//   liif_kernel; unfold_cells_kernel + metasr_kernel : the LIIF and MetaSR comparison decoders
//   axis_tables_kernel, sin_kernel : the device coordinate / sine code, exposed for tests.
// One compile-time hook that never ships enabled: DIINN_STAMPS (s_memtime stamps for tools/stamp_report.py).  The
// timing-ablation hooks of rounds 1-4 (ABL_*: wrong results by construction) were removed in round 5; the builds behind
// profiles/r0[1-4]_*ablation*.txt are reproducible from the commits of those rounds (git show 84fe2c6:<path>).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off  (explicit fmaf where wanted)
#include "diinn_device.h"
#include <stdlib.h>

struct TagCoopF { static constexpr bool value = false; };
struct TagCoopT { static constexpr bool value = true; };

// HEAD3 = true (decoder mode 4, diinn.py:89-90,140-147: last_layer = Conv2d(256, 3, 3, padding=1, 'reflect') over the HR grid): a
// 3x3 convolution of the 256-channel image q3 is a 1x1 map to 27 numbers per pixel, T[k][c] = sum_ch Lw[c][ch][ky][kx] q3[ch]
// (k = 3 ky + kx), followed by a 9-point gather (head3x3_reflect_kernel).  The first half depends on the pixel alone, so the layers
// run exactly as in mode 3 and the head forms 27 dot products in place of 3, in the same lane-half split and the same (m, g, e)
// order; they go to the TAP BUFFER p.out = [B][p.Orows rows from p.Orow0][Wu][TAP_STRIDE] (k major, c minor, one pad float: seven
// 16-byte stores per pixel).  The head table (27 x 256 floats, natural channel order) sits in LDS behind the Q0 rows of `tab`.
// (TAPS, TAP_STRIDE and the head image's layout: diinn_layout.h)
//
// INITQ = true (decoder init_q=True, mode 3: diinn.py:48-51,113-115): the unfolded features are multiplied by a per-pixel sine
// embedding before any layer sees them, so there is no per-cell P.  initq_planes_kernel (diinn_initq.hip) leaves, per HR PIXEL,
// PIX_CH = 1280 floats in p.P = [B][p.Prows HR rows from p.Prow0][Wu][1280]: channels 0..1023 are what P[cell] holds otherwise,
// channels 1024..1279 layer 0's sine argument (Q0 . E + bQ0, in revolutions).  Pc points at the pixel's own record, layer 0 reads
// its sine argument there and not from the Q0 table (whose rows the preamble skips); everything else is the code below as it is.
// INITQ rides in the first template argument, SIN_X = sine mode | DECODE_INITQ: the kernel keeps its four parameters, so every
// instantiation that existed before keeps its symbol name (and its instructions); the new ones are decode_kernel<SIN | DECODE_INITQ>.
//
// init_q with the other modes:
//   * modes 1/2, decode_kernel<SIN | DECODE_INITQ, KPART = false>: pixel_chain_kernel has written k_1..3 over channels 256..1023 of
//     the pixel's record, which the layers read as the multiplier exactly as they read the per-cell chain in P otherwise; with SAVE
//     (the training forward, diinn_decode_initq_train_fwd_qonly) it saves those k_i and the sine arguments in radians;
//   * mode 4, decode_kernel<SIN | DECODE_INITQ | DECODE_TAPS> (inference only): the tap form (HEAD3) reading the pixel's own record.  The tap form of
//     init_q rides in SIN_X too, NOT in the fourth template argument: the three decode_kernel<SIN, true, false, true> symbols stay
//     the only ones of that spelling (what picks mode 4's tap kernels out of the library by name keeps finding exactly those).
constexpr int DECODE_INITQ = 4;
constexpr int DECODE_TAPS = 8;
template <int SIN_X, bool KPART = true, bool SAVE = false, bool HEAD3_ARG = false>
__global__ __launch_bounds__(256, 1) void decode_kernel(const DecodeParams p) {
    constexpr int SIN_MODE = SIN_X & (DECODE_INITQ - 1);
    constexpr bool INITQ = (SIN_X & DECODE_INITQ) != 0;
    constexpr bool HEAD3 = HEAD3_ARG || (SIN_X & DECODE_TAPS) != 0;
    static_assert(SIN_X >= 0 && SIN_X < 2 * DECODE_TAPS && SIN_MODE <= DIINN_SIN_HW_REDUCED, "sine mode | DECODE_INITQ | DECODE_TAPS");
    static_assert(!(SIN_X & DECODE_TAPS) || (INITQ && !HEAD3_ARG), "DECODE_TAPS: the tap form of init_q only");
    static_assert(!(HEAD3 && SAVE), "mode 4 is inference only");
    // init_q: mode 3 and modes 1/2 (with SAVE: the planes are in radians, INITQ_RAD of initq_planes_kernel; modes 1/2 save the k_i
    // pixel_chain_kernel left in the record); mode 4's tap form is inference only (its training forward is mode 3's with SAVE)
    static_assert(!INITQ || !HEAD3 || (!SAVE && KPART), "init_q: modes 1-3, or mode 4's tap form without SAVE");
    // The small tables of layer 0 and of the head go through LDS: a vector-memory instruction blocks its wave for
    // ~60 cycles (stamps), and a wave reading them straight from the packed image issued 128 + 96
    // of those per tile.  Rows: Q0h, Q0w, t = fma(Q0r, ratio, bQ0) (the pixel-independent part of the sine
    // argument, the same first fma the per-pixel chain used to start with: results are bit-identical), L0, L1, L2.
    __shared__ __attribute__((aligned(16))) float tab[(HEAD3 ? 3 + TAPS : 6) * HID + 4];      // + the head bias bL
    // Inference (no SAVE) keeps the synthesis branch in REVOLUTIONS: weights, biases and the Q0 table come from the
    // sections divided by 2 pi (WLR, BQR, Q0R), so every sine is v_fract + v_sin instead of a 5-op reduction (each VALU
    // instruction costs ~3 cycles of fp32-MFMA issue).  The training forward saves sine arguments in radians and
    // stays on the plain sections.
    constexpr size_t S_WL = SAVE ? OFF_WL : OFF_WLR, S_BQ = SAVE ? OFF_BQ : OFF_BQR, S_Q0 = SAVE ? OFF_Q0 : OFF_Q0R;
    auto sine = [](float v) {
        if constexpr (SAVE) return dsin<SIN_MODE>(v); else return dsin_rev<SIN_MODE>(v);
    };
    {
        const int i = threadIdx.x & 63, part = threadIdx.x >> 6;
        const float* __restrict__ Q0s = p.Wt + S_Q0 + 4 * i;
        if (part == 0) {
            if constexpr (!INITQ) {
                *(f32x4*)(tab + 0 * HID + 4 * i) = *(const f32x4*)(Q0s + 0 * HID);
                *(f32x4*)(tab + 1 * HID + 4 * i) = *(const f32x4*)(Q0s + 1 * HID);
            }
        } else if (part == 1) {
            if constexpr (!INITQ) {
                const f32x4 wr = *(const f32x4*)(Q0s + 2 * HID), bq = *(const f32x4*)(Q0s + 3 * HID);
                f32x4 t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = __builtin_fmaf(wr[e], p.ratio, bq[e]);
                *(f32x4*)(tab + 2 * HID + 4 * i) = t;
            }
        } else if constexpr (HEAD3) {
            // (the 27 head rows are loaded by all four waves below; mode 4's bias and both validity words belong to the gather)
        } else if (part == 2) {
            *(f32x4*)(tab + 3 * HID + 4 * i) = *(const f32x4*)(p.Wt + OFF_L + 0 * HID + 4 * i);
            *(f32x4*)(tab + 4 * HID + 4 * i) = *(const f32x4*)(p.Wt + OFF_L + 1 * HID + 4 * i);
        } else {
            *(f32x4*)(tab + 5 * HID + 4 * i) = *(const f32x4*)(p.Wt + OFF_L + 2 * HID + 4 * i);
            if (i == 0) {                                        // bL + the image's validity word: inference reads derived
                const f32x4 bl = *(const f32x4*)(p.Wt + OFF_BL); // sections, so an image without them decodes to NaN
                // (the word is read on its own: hipcc 7.2 compiled `bit_cast<unsigned>(bl[3]) == MAGIC` on the scalarised
                // vector load into a compare of element 0)
                const unsigned nanm = SAVE ? 0u : derived_nan_mask(p.Wt);
                *(f32x4*)(tab + 6 * HID) = or_bits(bl, nanm);
            }
        }
        if constexpr (HEAD3) {
#pragma unroll
            for (int v = threadIdx.x; v < TAPS * HID / 4; v += 256)
                *(f32x4*)(tab + 3 * HID + 4 * v) = *(const f32x4*)(p.head3 + 4 * v);
        }
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform (scalar offsets)
    const int h = lane >> 5, j = lane & 31;

    int x, y, b;
    const long long ptile = (long long)blockIdx.x * 4 + wave;   // SAVE: plane tile of this wave
    if constexpr (SAVE) {                                        // 32 consecutive flattened pixels
        const long long pix = ptile * PLANE_TILE + j;
        const long long pc = pix < p.npix ? pix : p.npix - 1;    // lanes past the end compute on the last pixel
        const int hw = p.Hu * p.Wu;
        b = (int)(pc / hw);
        const int rem = (int)(pc - (long long)b * hw);
        y = rem / p.Wu;
        x = pix < p.npix ? rem - y * p.Wu : p.Wu;                // ... and are marked invalid below
    } else {
        x = p.x0 + blockIdx.x * (TILE_W * WG_TILES_X) + (wave & 1) * TILE_W + (j & (TILE_W - 1));
        y = p.y0 + blockIdx.y * (TILE_H * WG_TILES_Y) + (wave >> 1) * TILE_H + (j / TILE_W);
        b = blockIdx.z;
    }
    const bool valid = (x < p.x1) && (y < p.y1);
    __syncthreads();                                             // the tables are in LDS
    // whole wave outside the band/image: nothing to do (wave-uniform; no barrier follows)
    if (__builtin_amdgcn_readfirstlane((int)(__ballot(valid) == 0ull))) return;
    const int xc = x < p.Wu ? x : p.Wu - 1;
    const int yc = y < p.y1 ? y : p.y1 - 1;

    int iy, ix;
    float relh, relw;
    axis_eval(p.ah, yc, iy, relh);
    axis_eval(p.aw, xc, ix, relw);

#ifdef DIINN_STAMPS
    const size_t stamp_base = ((((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4 + wave) * 8;
    if (p.stamps && lane == 0) {
        unsigned long long rt;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt)::"memory");
        p.stamps[stamp_base + 7] = rt;
    }
#endif
    STAMP(0);
    const float* __restrict__ Wt = p.Wt;
    const float* __restrict__ Pc = INITQ ? p.P + (((size_t)b * p.Prows + (yc - p.Prow0)) * p.Wu + xc) * PIX_CH + 4 * h
                                         : p.P + (((size_t)b * p.Prows + (iy - p.Prow0)) * p.W + ix) * PCH + 4 * h;

    // saved-activation planes (SAVE): one buffer descriptor per layer covering this wave's plane tile
    // (512 rows x 32 pixels); a lane's offset is its pixel inside the row of channel 4h, the channel
    // row is a compile-time scalar offset.  Lanes past the end carry an offset outside the
    // descriptor's range: the store is dropped.
    const long long act_tiles = (p.npix + PLANE_TILE - 1) / PLANE_TILE;
    const unsigned act_voff = (SAVE && valid) ? 4u * j + 4u * h * PLANE_ROW_BYTES : 0xFFFFFFF0u;
    auto act_rsrc = [&](int layer) {
        return tile_rsrc(p.acts + (size_t)layer * act_tiles * ACT_ROWS * PLANE_TILE, ptile, ACT_ROWS);
    };

    // ---- layer 0: q0 = relu(P_0[cell]) * sin(Q0 . (rel_h, rel_w, ratio) + bQ0)   (diinn.py:133-134)
    float q[128];
    {
        const float* __restrict__ Q0 = tab + 4 * h;
        const __amdgpu_buffer_rsrc_t ar0 = act_rsrc(0);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * m + 8 * g;
                const f32x4 pv = *(const f32x4*)(Pc + c0);
                f32x4 wh, ww, tq;
                if constexpr (INITQ) {
                    tq = *(const f32x4*)(Pc + PCH + c0);         // the pixel's own sine argument
                } else {
                    wh = *(const f32x4*)(Q0 + 0 * HID + c0);
                    ww = *(const f32x4*)(Q0 + 1 * HID + c0);
                    tq = *(const f32x4*)(Q0 + 2 * HID + c0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float a = tq[e];
                    if constexpr (!INITQ) {
                        a = __builtin_fmaf(ww[e], relw, a);
                        a = __builtin_fmaf(wh[e], relh, a);
                    }
                    const float kv = relu0(pv[e]);
                    q[16 * m + 4 * g + e] = kv * sine(a);
                    if constexpr (SAVE) {
                        st_act(ar0, act_voff, (unsigned)(c0 + e) * PLANE_ROW_BYTES, kv);
                        st_act(ar0, act_voff, (unsigned)(HID + c0 + e) * PLANE_ROW_BYTES, a);
                    }
                }
            }
        }
    }

    STAMP(1);
    // ---- layers 1..3: [k;s] = [Wq_i;Qw_i] . q + [P_i[cell]; bQ_i];  q = relu(k) * sin(s)   (diinn.py:135-137)
    // Software pipeline, spelled out in program order (the loops below are fully unrolled):
    //   * weight pieces are fetched PF steps (8 MFMAs = 512 cycles each) ahead into a register ring
    //     that is carried across tiles and layers (the packed image is contiguous in step order);
    //   * the accumulator seeds of tile m+1 (P_i[cell], bQ_i) are fetched during tile m;
    //   * the VALU epilogue (relu * sin) of tile m-1 is spread over the MFMA stream of tile m.
    constexpr int PF = DECODE_PREFETCH;
    static_assert(WL_KG % PF == 0, "ring index must be static");
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)Wt, 0, (int)(PACKED_FLOATS * sizeof(float)), 0x00020000);   // reads past the end return 0
    const int lane_off = lane * 16;
    int wp = (int)(S_WL * sizeof(float));                        // byte offset; advances one layer per iteration
    f32x4 rk[PF], rq[PF];
#pragma unroll
    for (int d = 0; d < PF; ++d) {
        if constexpr (KPART) rk[d] = ld_piece(wrs, lane_off, wp + (2 * d + 0) * PIECE_BYTES);
        rq[d] = ld_piece(wrs, lane_off, wp + (2 * d + 1) * PIECE_BYTES);
    }
    f32x4 sk[4], sq[4];                                          // seeds of the next tile
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        sk[g] = *(const f32x4*)(Pc + HID + 8 * g);
        sq[g] = *(const f32x4*)(Wt + S_BQ + 4 * h + 8 * g);
    }
#pragma unroll 1
    for (int layer = 0; layer < 3; ++layer) {
        const int nl = layer < 2 ? layer + 1 : 2;                // seeds of the next layer's tile 0 (clamped)
        const float* __restrict__ Pl = Pc + (layer + 1) * HID;
        const float* __restrict__ Bq = Wt + S_BQ + layer * HID + 4 * h;
        const float* __restrict__ Pn = Pc + (nl + 1) * HID;
        const float* __restrict__ Bn = Wt + S_BQ + nl * HID + 4 * h;
        float qn[128];
        f32x16 pk, ps;                                           // finished accumulators of the previous tile
        const __amdgpu_buffer_rsrc_t arl = act_rsrc(layer + 1);
        (void)arl;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            f32x16 ak, as;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ak[4 * g + e] = sk[g][e];
                    as[4 * g + e] = sq[g][e];
                }
            }
#pragma unroll
            for (int kg = 0; kg < WL_KG; ++kg) {
                const int s = m * WL_KG + kg;
                const f32x4 wq = rq[s % PF];
                if constexpr (KPART) {
                    const f32x4 wk = rk[s % PF];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        ak = MFMA32(wk[e], q[4 * kg + e], ak);
                        as = MFMA32(wq[e], q[4 * kg + e], as);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) as = MFMA32(wq[e], q[4 * kg + e], as);
                }
                // refill the ring slot just consumed with the piece PF steps ahead
                if constexpr (KPART) rk[s % PF] = ld_piece(wrs, lane_off, wp + (2 * (s + PF) + 0) * PIECE_BYTES);
                rq[s % PF] = ld_piece(wrs, lane_off, wp + (2 * (s + PF) + 1) * PIECE_BYTES);
                if (kg == 4) {                                    // seeds for the next tile
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        sk[g] = *(const f32x4*)((m < 7 ? Pl + 32 * (m + 1) : Pn) + 8 * g);
                        sq[g] = *(const f32x4*)((m < 7 ? Bq + 32 * (m + 1) : Bn) + 8 * g);
                    }
                }
                if (m > 0 && (kg & 1) == 0) {                     // one epilogue element of tile m-1 every 16 MFMAs
                    const int r = kg >> 1;
                    const float kv = relu0(pk[r]);
                    qn[16 * (m - 1) + r] = kv * sine(ps[r]);
                    if constexpr (SAVE) {                        // register r of tile m-1 = channel 32(m-1) + (r&3) + 8(r>>2) + 4h
                        const unsigned so = (unsigned)(32 * (m - 1) + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES;
                        st_act(arl, act_voff, so, kv);
                        st_act(arl, act_voff, so + HID * PLANE_ROW_BYTES, ps[r]);
                    }
                }
            }
            pk = ak;
            ps = as;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float kv = relu0(pk[r]);
            qn[16 * 7 + r] = kv * sine(ps[r]);
            if constexpr (SAVE) {
                const unsigned so = (unsigned)(32 * 7 + (r & 3) + 8 * (r >> 2)) * PLANE_ROW_BYTES;
                st_act(arl, act_voff, so, kv);
                st_act(arl, act_voff, so + HID * PLANE_ROW_BYTES, ps[r]);
            }
        }
#pragma unroll
        for (int i = 0; i < 128; ++i) q[i] = qn[i];
        wp += (int)(WL_LAYER * sizeof(float));
#ifdef DIINN_STAMPS
        if (layer == 0) STAMP(2); else if (layer == 1) STAMP(3); else STAMP(4);
#endif
    }

    if constexpr (HEAD3) {
        // ---- mode 4: the 27 tap values T[k][c] = Lw[c][:][ky][kx] . q3 of this pixel   (diinn.py:146, first half)
        float o[TAPS];
#pragma unroll
        for (int r = 0; r < TAPS; ++r) o[r] = 0.0f;
        const float* __restrict__ L = tab + 3 * HID + 4 * h;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * m + 8 * g;
#pragma unroll
                for (int r = 0; r < TAPS; ++r) {
                    const f32x4 l = *(const f32x4*)(L + r * HID + c0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[r] = __builtin_fmaf(l[e], q[16 * m + 4 * g + e], o[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < TAPS; ++r) o[r] += __shfl_xor(o[r], 32);
        if (valid && h == 0) {
            float* t = p.out + (((long long)b * p.Orows + (y - p.Orow0)) * p.Wu + x) * TAP_STRIDE;
#pragma unroll
            for (int v = 0; v < TAP_STRIDE / 4; ++v)
                *(f32x4*)(t + 4 * v) = f32x4{o[4 * v], o[4 * v + 1], o[4 * v + 2], 4 * v + 3 < TAPS ? o[(4 * v + 3) % TAPS] : 0.0f};
        }
        STAMP(5);
        return;
    }
    // ---- head: out = L . q3 + bL   (diinn.py:138)
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    {
        const float* __restrict__ L = tab + 3 * HID + 4 * h;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * m + 8 * g;
                const f32x4 l0 = *(const f32x4*)(L + 0 * HID + c0);
                const f32x4 l1 = *(const f32x4*)(L + 1 * HID + c0);
                const f32x4 l2 = *(const f32x4*)(L + 2 * HID + c0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = q[16 * m + 4 * g + e];
                    o0 = __builtin_fmaf(l0[e], v, o0);
                    o1 = __builtin_fmaf(l1[e], v, o1);
                    o2 = __builtin_fmaf(l2[e], v, o2);
                }
            }
        }
    }
    o0 += __shfl_xor(o0, 32);
    o1 += __shfl_xor(o1, 32);
    o2 += __shfl_xor(o2, 32);
    if (valid && h == 0) {
        const long long plane = p.o_ps;
        float* o = out_px(p, b, y, x);
        o[0] = o0 + tab[6 * HID + 0];
        o[plane] = o1 + tab[6 * HID + 1];
        o[2 * plane] = o2 + tab[6 * HID + 2];
    }
    STAMP(5);
}



// ---------------------------------------------------------------------------------
// decode_coop16_kernel: the fp32 latency form for small and partly filled launches (BASELINE config 1: 96 x 96).
// decode_kernel gives one wave a 32-pixel tile and 6,144 dependent MFMAs (0.165 ms at any size).  (Round 2's form -- four
// waves sharing ONE 32-pixel tile, a chain of 3 x 512 MFMAs of 64 clocks, 41 us -- never won against this one and was
// deleted in round 5: DESIGN_HISTORY.md.)  Here a workgroup owns a
// 4 x 4 = 16-pixel tile on v_mfma_f32_16x16x4_f32 (32 clocks): wave w owns output channels 64 w .. 64 w + 63 of both
// branches as four 16-row M-tiles each (8 accumulators of 4 registers, 512 MFMAs per layer, 20 us per tile), twice
// the workgroups at half the chain, four workgroups per CU (38 KiB of LDS, < 128 registers).  Measured at c1 (r04,
// profiles/r04_c1_latency.txt): decode 0.099 -> 0.076-0.079 ms, step 0.122 -> 0.100-0.102 ms.  What bounds it now is the
// makespan of 576 tiles on 256 CUs (three per busiest CU x ~23 us); capping the workgroups per CU at 3 or 2, weights kept
// L1-resident, or no weight requests at all (timing ablations) move it by < 4 %.
//   * A operands: packed section 16 (WL16), [i][half][lane][T]: a k-step's two 1 KiB pieces feed its 8 MFMAs;
//   * B operand: the activation in LDS in POSITION order -- position p = the p-th term of decode_kernel's accumulation
//     chain, channel chan_of(p >> 1, p & 1) -- as [p >> 4][16 (p & 3) + pixel][(p >> 2) & 3]: lane (g, n) reads the
//     four k-steps 4 ib .. 4 ib + 3 of its k = g with one ds_read_b128;
//   * per output channel the arithmetic is decode_kernel's: same seed, the same k-ordered chain (the 16x16x4 MFMA adds
//     its four products in k order like the 32x32x2 one adds its two: tests hold the two kernels bit-equal), same
//     epilogue, and wave 0 runs decode_kernel's head order on the last activation.
// ---------------------------------------------------------------------------------
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
constexpr int T16_W = 4, T16_H = 4;

template <int SIN_MODE>
__global__ __launch_bounds__(256, 4) void decode_coop16_kernel(const DecodeParams p) {
    __shared__ __attribute__((aligned(16))) f32x4 qs[2][16][64];           // 2 x 16 KiB: activation in position order
    __shared__ __attribute__((aligned(16))) float tab[6 * HID + 4];        // Q0h, Q0w, fma(Q0r, ratio, bQ0), L0..L2, bL
    {
        const int i = threadIdx.x & 63, part = threadIdx.x >> 6;
        const float* __restrict__ Q0s = p.Wt + OFF_Q0R + 4 * i;
        if (part == 0) {
            *(f32x4*)(tab + 0 * HID + 4 * i) = *(const f32x4*)(Q0s + 0 * HID);
            *(f32x4*)(tab + 1 * HID + 4 * i) = *(const f32x4*)(Q0s + 1 * HID);
        } else if (part == 1) {
            const f32x4 wr = *(const f32x4*)(Q0s + 2 * HID), bq = *(const f32x4*)(Q0s + 3 * HID);
            f32x4 t;
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = __builtin_fmaf(wr[e], p.ratio, bq[e]);
            *(f32x4*)(tab + 2 * HID + 4 * i) = t;
        } else if (part == 2) {
            *(f32x4*)(tab + 3 * HID + 4 * i) = *(const f32x4*)(p.Wt + OFF_L + 0 * HID + 4 * i);
            *(f32x4*)(tab + 4 * HID + 4 * i) = *(const f32x4*)(p.Wt + OFF_L + 1 * HID + 4 * i);
        } else {
            *(f32x4*)(tab + 5 * HID + 4 * i) = *(const f32x4*)(p.Wt + OFF_L + 2 * HID + 4 * i);
            if (i == 0) *(f32x4*)(tab + 6 * HID) = or_bits(*(const f32x4*)(p.Wt + OFF_BL), derived_nan_mask(p.Wt));
        }
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, n = lane & 15;
    const int x = p.x0 + blockIdx.x * T16_W + (n & (T16_W - 1));
    const int y = p.y0 + blockIdx.y * T16_H + (n / T16_W);
    const int b = blockIdx.z;
    const bool valid = (x < p.x1) && (y < p.y1);
    const int xc = x < p.Wu ? x : p.Wu - 1;
    const int yc = y < p.y1 ? y : p.y1 - 1;
    int iy, ix;
    float relh, relw;
    axis_eval(p.ah, yc, iy, relh);
    axis_eval(p.aw, xc, ix, relw);
    const float* __restrict__ Wt = p.Wt;
    // this lane's channels: 64 wave + 16 T + 4 g + j (T, j = 0..3) = accumulator register j of M-tile T
    const float* __restrict__ Pc = p.P + (((size_t)b * p.Prows + (iy - p.Prow0)) * p.W + ix) * PCH + 64 * wave + 4 * g;
    // where channel 64 wave + 16 T + 4 g + j goes in a position-ordered image (floats): base + 256 T + {0, 128, 1, 129}[j]
    // (position 32 m + 8 a + 2 j + h with m = 2 wave + (T >> 1), a = 2 (T & 1) + (g >> 1), h = g & 1)
    float* const qf = reinterpret_cast<float*>(&qs[0][0][0]);
    const int wbase = (4 * wave * 64 + 16 * (g & 1) + n) * 4 + 2 * (g >> 1);
    auto put = [&](const int img, const int T, const f32x4 v) {
        float* d = qf + img * (16 * 64 * 4) + wbase + 256 * T;
        d[0] = v[0]; d[128] = v[1]; d[1] = v[2]; d[129] = v[3];
    };
    __syncthreads();

    // ---- layer 0 (diinn.py:133-134), decode_kernel's operation order
#pragma unroll
    for (int T = 0; T < 4; ++T) {
        const int c0 = 64 * wave + 16 * T + 4 * g;
        const f32x4 pv = *(const f32x4*)(Pc + 16 * T);
        const f32x4 wh = *(const f32x4*)(tab + 0 * HID + c0);
        const f32x4 ww = *(const f32x4*)(tab + 1 * HID + c0);
        const f32x4 tq = *(const f32x4*)(tab + 2 * HID + c0);
        f32x4 q0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = tq[e];
            a = __builtin_fmaf(ww[e], relw, a);
            a = __builtin_fmaf(wh[e], relh, a);
            q0[e] = relu0(pv[e]) * dsin_rev<SIN_MODE>(a);
        }
        put(0, T, q0);
    }

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)Wt, 0, (int)(PACKED_FLOATS * sizeof(float)), 0x00020000);
    const int lane_off = lane * 16;
    int wp = (int)(OFF_WL16 * sizeof(float)) + wave * (int)(WL16_WAVE * sizeof(float));
    auto ld_w = [&](const int i, const int half) {
        return ld_piece(wrs, lane_off, wp + (2 * i + half) * PIECE_BYTES);
    };
    __syncthreads();

    // The weight ring (RING - 1 k-steps of two pieces in flight; 8 MFMAs = 256 clocks per k-step) and the accumulator seeds
    // run on ACROSS the layers: the last steps of a layer request the next layer's first pieces, and its seeds (P_{i+1} of
    // the pixel's cell, bQ) are requested in the middle of the layer before -- nothing a layer needs is fetched at its start.
    constexpr int RING = 4;
    f32x4 rw[RING][2];
#pragma unroll
    for (int d = 0; d < RING - 1; ++d) {
        rw[d][0] = ld_w(d, 0);
        rw[d][1] = ld_w(d, 1);
    }
    f32x4 seed[8];
    auto ld_seeds = [&](const int layer) {
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            seed[T] = *(const f32x4*)(Pc + (layer + 1) * HID + 16 * T);
            seed[4 + T] = *(const f32x4*)(Wt + OFF_BQR + layer * HID + 64 * wave + 16 * T + 4 * g);
        }
    };
    ld_seeds(0);
    auto layer_body = [&](auto cur_tag, auto last_tag, const int layer) {
        constexpr int CUR = decltype(cur_tag)::value ? 1 : 0;
        constexpr bool LAST = decltype(last_tag)::value;
        f32x4 acc[8];                                            // [T]: modulation, [4 + T]: synthesis
#pragma unroll
        for (int T = 0; T < 8; ++T) acc[T] = seed[T];
        f32x4 bq = qs[CUR][0][lane];
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const float bv = bq[i & 3];
            if ((i & 3) == 3 && i + 1 < 64) bq = qs[CUR][(i + 1) >> 2][lane];
            if (i + RING - 1 < 64) {
                rw[(i + RING - 1) % RING][0] = ld_w(i + RING - 1, 0);
                rw[(i + RING - 1) % RING][1] = ld_w(i + RING - 1, 1);
            } else if (!LAST) {                                  // the next layer's first k-steps (64 % RING == 0: same slots)
                rw[(i + RING - 1) % RING][0] = ld_w(i + RING - 1 + (int)(WL16_LAYER / WL16_KSTEP) - 64, 0);
                rw[(i + RING - 1) % RING][1] = ld_w(i + RING - 1 + (int)(WL16_LAYER / WL16_KSTEP) - 64, 1);
            }
            if (i == 32 && !LAST) ld_seeds(layer + 1);
#pragma unroll
            for (int T = 0; T < 4; ++T) {
                acc[T] = MFMA16(rw[i % RING][0][T], bv, acc[T]);
                acc[4 + T] = MFMA16(rw[i % RING][1][T], bv, acc[4 + T]);
            }
            // a k-step's two requests stay RING - 1 steps (768 clocks of MFMAs) ahead of their use: left alone, hipcc sinks
            // every load to 4 MFMAs in front of its first use and the wave waits for the L2 at each step
            __builtin_amdgcn_sched_barrier(0);
        }
        // epilogue: q = relu(k) * sin(s) for this wave's 64 channels -> the other image
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            f32x4 qn;
#pragma unroll
            for (int e = 0; e < 4; ++e) qn[e] = relu0(acc[T][e]) * dsin_rev<SIN_MODE>(acc[4 + T][e]);
            put(1 - CUR, T, qn);
        }
        __syncthreads();
    };
    static_assert(64 % RING == 0 && WL16_LAYER == 4 * WL16_WAVE && WL16_WAVE == 64 * WL16_KSTEP, "ring runs on across layers");
    layer_body(TagCoopF{}, TagCoopF{}, 0);                       // image 0 -> 1
    wp += (int)(WL16_LAYER * sizeof(float));
    layer_body(TagCoopT{}, TagCoopF{}, 1);                       // 1 -> 0
    wp += (int)(WL16_LAYER * sizeof(float));
    layer_body(TagCoopF{}, TagCoopT{}, 2);                       // 0 -> 1

    // ---- head (diinn.py:138): decode_kernel's order -- per lane half h the channels 32 m + 8 gq + 4 h + e in (m, gq, e)
    // order, then the two halves added -- on the last activation (image 1), by lanes (h, n) of wave 0
    if (wave == 0 && lane < 32) {
        const int h = lane >> 4;
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        const float* __restrict__ L = tab + 3 * HID + 4 * h;
        const float* __restrict__ q1 = qf + 16 * 64 * 4 + (16 * h + n) * 4;     // position 32 m + 8 gq + 2 e + h
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int c0 = 32 * m + 8 * gq;
                const f32x4 l0 = *(const f32x4*)(L + 0 * HID + c0);
                const f32x4 l1 = *(const f32x4*)(L + 1 * HID + c0);
                const f32x4 l2 = *(const f32x4*)(L + 2 * HID + c0);
                // positions 32 m + 8 gq + 2 e + h: image row 2 m + (gq >> 1), lane group 2 (e & 1) + h, element 2 (gq & 1) + (e >> 1)
                const float* __restrict__ r = q1 + (2 * m + (gq >> 1)) * 256 + 2 * (gq & 1);
                const float v[4] = {r[0], r[128], r[1], r[129]};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o0 = __builtin_fmaf(l0[e], v[e], o0);
                    o1 = __builtin_fmaf(l1[e], v[e], o1);
                    o2 = __builtin_fmaf(l2[e], v[e], o2);
                }
            }
        }
        o0 += __shfl_xor(o0, 16);
        o1 += __shfl_xor(o1, 16);
        o2 += __shfl_xor(o2, 16);
        if (valid && h == 0) {
            const long long plane = p.o_ps;
            float* op = out_px(p, b, y, x);
            op[0] = o0 + tab[6 * HID + 0];
            op[plane] = o1 + tab[6 * HID + 1];
            op[2 * plane] = o2 + tab[6 * HID + 2];
        }
    }
}

// ---------------------------------------------------------------------------------
// cell_chain_kernel (decoder modes 1 and 2, diinn.py:116-131): the modulation chain depends on the
// LR cell only: k_0 = relu(P_0), k_i = relu(K_i^k k_{i-1} + P_i), i = 1..3.  Same register-resident
// scheme as decode_kernel with LR cells in place of HR pixels and the modulation half of the
// stacked weights alone (part 0 of the WL image holds K.i[:, :256] in A-operand order already).
// k_i overwrites the P_i slot of the workspace; decode_kernel<SIN, KPART=false> then reads it as
// the multiplier of the synthesis branch.
// ---------------------------------------------------------------------------------
struct ChainParams {
    float* P;            // [B,Prows,W,1024] = LR rows [Prow0, Prow0+Prows); slots 1..3 updated in place for rows [r0,r1)
    const float* Wt;
    int B, H, W, r0, r1, Prow0, Prows;
};

// The chain of one wave's 32 records (shared by cell_chain_kernel and pixel_chain_kernel): Pc = the lane's record + 4 h, the
// first 1024 floats of which are the four 256-channel slots.  BK_SEEDS: layers 1..3 are seeded from bK_i of the packed image
// (slots 1..3 of the record are written, never read); otherwise from the slot itself, which k_i then overwrites.
template <bool BK_SEEDS>
__device__ __forceinline__ void chain_body(float* __restrict__ Pc, const float* Wt, const bool valid, const int lane, const int h) {
    float k[128];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const f32x4 pv = *(const f32x4*)(Pc + 8 * i);             // channels 32m + 8g + 4h .., i = 4m + g
#pragma unroll
        for (int e = 0; e < 4; ++e) k[4 * i + e] = relu0(pv[e]);
    }

    constexpr int PF = DECODE_PREFETCH;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)Wt, 0, (int)(PACKED_FLOATS * sizeof(float)), 0x00020000);
    const int lane_off = lane * 16;
    int wp = (int)(OFF_WL * sizeof(float));
    f32x4 rk[PF];
#pragma unroll
    for (int d = 0; d < PF; ++d) rk[d] = ld_piece(wrs, lane_off, wp + (2 * d) * PIECE_BYTES);
#pragma unroll 1
    for (int layer = 0; layer < 3; ++layer) {
        float* __restrict__ Pl = Pc + (layer + 1) * HID;
        float kn[128];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            f32x16 ak;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 pv;
                if constexpr (BK_SEEDS) pv = *(const f32x4*)(Wt + OFF_BK + (layer + 1) * HID + 4 * h + 32 * m + 8 * g);
                else pv = *(const f32x4*)(Pl + 32 * m + 8 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) ak[4 * g + e] = pv[e];
            }
#pragma unroll
            for (int kg = 0; kg < WL_KG; ++kg) {
                const int s = m * WL_KG + kg;
                const f32x4 wk = rk[s % PF];
#pragma unroll
                for (int e = 0; e < 4; ++e) ak = MFMA32(wk[e], k[4 * kg + e], ak);
                rk[s % PF] = ld_piece(wrs, lane_off, wp + (2 * (s + PF)) * PIECE_BYTES);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = relu0(ak[4 * g + e]);
                    kn[16 * m + 4 * g + e] = v[e];
                }
                if (valid) *(f32x4*)(Pl + 32 * m + 8 * g) = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 128; ++i) k[i] = kn[i];
        wp += (int)(WL_LAYER * sizeof(float));
    }
}

__global__ __launch_bounds__(256, 1) void cell_chain_kernel(const ChainParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int x = blockIdx.x * (TILE_W * WG_TILES_X) + (wave & 1) * TILE_W + (j & (TILE_W - 1));
    const int y = p.r0 + blockIdx.y * (TILE_H * WG_TILES_Y) + (wave >> 1) * TILE_H + (j / TILE_W);
    const int b = blockIdx.z;
    const bool valid = (x < p.W) && (y < p.r1);
    if (__builtin_amdgcn_readfirstlane((int)(__ballot(valid) == 0ull))) return;
    const int xc = x < p.W ? x : p.W - 1;
    const int yc = y < p.r1 ? y : p.r1 - 1;
    float* __restrict__ Pc = p.P + (((size_t)b * p.Prows + (yc - p.Prow0)) * p.W + xc) * PCH + 4 * h;
    chain_body<false>(Pc, p.Wt, valid, lane, h);
}

// ---------------------------------------------------------------------------------
// pixel_chain_kernel (decoder modes 1 and 2 with init_q=True, diinn.py:113-131): x' = E * X[cell] depends on the HR pixel, so the
// modulation chain does too.  cell_chain_kernel's scheme with the HR pixels of a chunk in place of LR cells and the pixel
// records of initq_planes_kernel (stride PIX_CH) in place of P: k_i = relu(K_i[:, :256] k_{i-1} + seed_i) overwrites channels
// 256 i .. 256 i + 255 of the pixel's record, and decode_kernel<SIN | DECODE_INITQ, KPART = false> reads it as the multiplier.
// seed_i is the slot itself (mode 2: Wx_i . x' + bK_i from the 1280-row planes) or, BK_SEEDS (mode 1, the 512-row planes, which
// leave those slots unwritten), bK_i from the packed image.  A lane past the chunk's edge computes on a record of its own wave
// and stores nothing (as in cell_chain_kernel).  No atomics, no scratch; a pixel's arithmetic depends on the pixel alone.
// ---------------------------------------------------------------------------------
struct PixChainParams {
    float* pix;          // [B][rows][Wu][PIX_CH]: the pixel planes of one chunk of HR rows
    const float* Wt;
    int B, Wu, rows;
};

template <bool BK_SEEDS>
__global__ __launch_bounds__(256, 1) void pixel_chain_kernel(const PixChainParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int x = blockIdx.x * (TILE_W * WG_TILES_X) + (wave & 1) * TILE_W + (j & (TILE_W - 1));
    const int y = blockIdx.y * (TILE_H * WG_TILES_Y) + (wave >> 1) * TILE_H + (j / TILE_W);
    const int b = blockIdx.z;
    const bool valid = (x < p.Wu) && (y < p.rows);
    if (__builtin_amdgcn_readfirstlane((int)(__ballot(valid) == 0ull))) return;
    const int xc = x < p.Wu ? x : p.Wu - 1;
    const int yc = y < p.rows ? y : p.rows - 1;
    float* __restrict__ Pc = p.pix + (((size_t)b * p.rows + yc) * p.Wu + xc) * PIX_CH + 4 * h;
    chain_body<BK_SEEDS>(Pc, p.Wt, valid, lane, h);
}

static int pixel_chain_impl(void* stream, float* pix_dev, const float* packed_dev, int B, int Wu, int rows, bool bk_seeds) {
    if (!all_set(pix_dev, packed_dev)) return DIINN_ERR_INVALID_ARG;
    if (B <= 0 || Wu <= 0 || rows <= 0) return DIINN_ERR_INVALID_ARG;
    if ((((size_t)pix_dev) | ((size_t)packed_dev)) & 15) return DIINN_ERR_INVALID_ARG;      // 16-byte seeds and pieces
    if (int st = check_extent(rows, Wu)) return st;
    const dim3 grid(grid_blocks(0, Wu, WG_W), grid_blocks(0, rows, WG_H), B);
    if (int st = check_grid(grid.y, B)) return st;
    const PixChainParams p{pix_dev, packed_dev, B, Wu, rows};
    pick<1, 0>(bk_seeds, [&](auto S) {
        hipLaunchKernelGGL(pixel_chain_kernel<decltype(S)::value>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
    return hip_status(hipGetLastError());
}

static int cell_chain_impl(void* stream, float* P_dev, const float* packed_dev, int B, int H, int W, int r0, int r1,
                           RowWin pw) {
    if (!all_set(P_dev, packed_dev)) return DIINN_ERR_INVALID_ARG;
    if (int st = check_dims(B, H, W)) return st;
    if (r0 < 0 || r1 > H || r0 >= r1) return DIINN_ERR_INVALID_ARG;
    if (int st = check_window(pw.row0, pw.rows, H, r0, r1)) return st;
    ChainParams p{P_dev, packed_dev, B, H, W, r0, r1, pw.row0, pw.rows};
    const dim3 grid(grid_blocks(0, W, WG_W), grid_blocks(r0, r1, WG_H), B);
    if (int st = check_grid(grid.y, B)) return st;
    hipLaunchKernelGGL(cell_chain_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

// Where the pixels of a launch go: `out` points at pixel (b = 0, c = 0, y = row0, x = col0) of the caller's buffer, the
// strides are in floats.  The row-band entry points describe a contiguous [B,3,rows,Wu] window this way (contig()).
struct OutView { int row0, rows, col0; long long bs, ps, rs; };
static inline OutView contig(RowWin ow, int Wu) {
    return OutView{ow.row0, ow.rows, 0, 3LL * ow.rows * Wu, (long long)ow.rows * Wu, (long long)Wu};
}

// The one place a DecodeParams is filled: HR rows [y0,y1) x columns [x0,x1) of the Hu x Wu image of a B x H x W map, P holding
// rows `pw` (LR rows of the hoisted conv -- or HR rows, where P is init_q's pixel planes), the pixels going to `ov`.  Every
// member a launch does not name is zero: the caller adds what is its own (acts / npix, head3, split, the stamp buffer) and
// the bf16 launchers their seed_cols / xcd_runs / pg.
static DecodeParams decode_params(const float* P_dev, const float* packed_dev, float* out_dev, int B, int H, int W, int Hu, int Wu,
                                  int y0, int y1, int x0, int x1, RowWin pw, OutView ov) {
    DecodeParams p{};
    p.P = P_dev; p.Wt = packed_dev; p.out = out_dev;
    p.B = B; p.H = H; p.W = W; p.Hu = Hu; p.Wu = Wu; p.y0 = y0; p.y1 = y1;
    p.Prow0 = pw.row0; p.Prows = pw.rows; p.Orow0 = ov.row0; p.Orows = ov.rows;
    p.x0 = x0; p.x1 = x1; p.Ocol0 = ov.col0; p.o_bs = ov.bs; p.o_ps = ov.ps; p.o_rs = ov.rs;
    p.ratio = (float)(((double)H * (double)W) / ((double)Hu * (double)Wu));
    const int small = diinn_uses_small_output_kernel(Hu, Wu);
    p.ah = make_axis(H, Hu, small);
    p.aw = make_axis(W, Wu, small);
    return p;
}
static inline dim3 decode_grid(int B, int y0, int y1, int x0, int x1) {   // workgroups of 16 x 8 pixels anchored at (x0, y0)
    return dim3(grid_blocks(x0, x1, WG_W), grid_blocks(y0, y1, WG_H), B);
}

// HR rows [y0,y1) x columns [x0,x1) of the image, every arithmetic mode.  Blocks are anchored at (x0, y0); no pixel's
// arithmetic depends on its place in a block, and every kernel-variant choice that is not bit-neutral is made from the
// FULL image, so a tile is bit-identical to the same pixels of a whole-image decode.
// Which fp32 kernel a tile launch takes, and its grid (one function for the launch and for diinn_decode_kernel_info).
// decode_kernel runs whole ROUNDS of one workgroup of 16 x 8 pixels per compute unit, 181 us each whatever the fill; the
// 16-pixel latency kernel is work-conserving (four workgroups per CU) at 0.0896 us per tile on 256 CUs + ~25 us -- 1.3 %
// behind on exact rounds (c2: 5.87 vs 5.79 ms), far ahead on a partly filled last round (48 -> 192: 0.234 vs 0.363 ms;
// r04, tools/f32_kernel_choice.py, profiles/r04_f32_kernel_choice.txt).  The launch takes the cheaper by that model, with
// the device's own CU count in it.  DIINN_F32_KERNEL = 1 / 3 forces the throughput / the 16-pixel latency kernel (tests,
// A-B timing).
struct F32Choice { int kernel; dim3 grid; };
static F32Choice f32_kernel_choice(int B, int y0, int y1, int x0, int x1) {
    const dim3 grid = decode_grid(B, y0, y1, x0, x1);
    const int force = (int)knob(diinn_knobs().f32_kernel);
    const int ncu = device_cus();
    const dim3 grid16(grid_blocks(x0, x1, T16_W), grid_blocks(y0, y1, T16_H), B);
    const double t16 = (double)grid16.x * grid16.y * grid16.z, rounds = (double)(((long long)grid.x * grid.y * B + ncu - 1) / ncu);
    const bool cheaper16 = 0.0896 * t16 * (256.0 / ncu) + 25.0 < 181.1 * rounds + 3.0;
    if (grid16.y <= 65535 && (force ? force == 3 : cheaper16)) return F32Choice{DIINN_DECODE_KERNEL_LATENCY16, grid16};
    return F32Choice{DIINN_DECODE_KERNEL_THROUGHPUT, grid};
}

static int decode_tile_impl(void* stream, const float* P_dev, const float* packed_dev,
                            float* out_dev, int B, int H, int W, int Hu, int Wu,
                            int y0, int y1, int x0, int x1, int sin_mode, int compute, RowWin pw, OutView ov,
                            bool x3q = false) {
    if (!compute_ok(compute)) return DIINN_ERR_UNSUPPORTED;      // (this entry point's order: the arithmetic first)
    if (!all_set(P_dev, packed_dev, out_dev)) return DIINN_ERR_INVALID_ARG;
    if (int st = check_dims(B, H, W)) return st;
    if (int st = check_band(Hu, Wu, y0, y1)) return st;
    if (x0 < 0 || x1 > Wu || x0 >= x1) return DIINN_ERR_INVALID_ARG;
    if (int st = check_extent(Hu, Wu)) return st;
    int r0, r1;
    if (int st = diinn_lr_rows_for_band(H, Hu, Wu, y0, y1, &r0, &r1)) return st;
    if (int st = check_window(pw.row0, pw.rows, H, r0, r1)) return st;
    if (int st = check_window(ov.row0, ov.rows, Hu, y0, y1)) return st;
    // strides: a row holds the tile's columns, a plane its rows, a batch item its three planes (no overlap); < 2^40 floats
    if (ov.col0 < 0 || ov.col0 > x0 || ov.rs < (long long)(x1 - ov.col0) || ov.ps < ov.rs * (y1 - ov.row0 - 1) + (x1 - ov.col0) ||
        ov.bs < 2 * ov.ps + ov.rs * (y1 - ov.row0 - 1) + (x1 - ov.col0) || ov.bs > (1LL << 40))
        return DIINN_ERR_INVALID_ARG;
    if (int st = check_sin(sin_mode)) return st;
    const dim3 grid = decode_grid(B, y0, y1, x0, x1);
    if (int st = check_grid(grid.y, grid.z)) return st;
    DecodeParams p = decode_params(P_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, x0, x1, pw, ov);
#ifdef DIINN_STAMPS
    p.stamps = g_stamps;
#endif
    if (compute == DIINN_COMPUTE_BF16 || compute == DIINN_COMPUTE_BF16_FULL)
        return launch_decode_bf16(stream, p, grid.x, grid.y, grid.z, sin_mode);
    if (compute == DIINN_COMPUTE_BF16X3)
        return launch_decode_bf16x3(stream, p, grid.x, grid.y, grid.z, sin_mode);
    if (compute == DIINN_COMPUTE_F32_QONLY && x3q)              // modes 1/2, the synthesis branch in split bf16
        return launch_decode_bf16x3_form(stream, p, grid, sin_mode, X3_QONLY);
    if (compute == DIINN_COMPUTE_F32_QONLY)
        return launch_sin(sin_mode, [&](auto S) {
            hipLaunchKernelGGL((decode_kernel<decltype(S)::value, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
        });
    // Which of the two fp32 kernels (bit-equal: tests/test_gpu_parity.py::test_latency_kernel_is_bit_identical_...)?
    const F32Choice ch = f32_kernel_choice(B, y0, y1, x0, x1);
    if (ch.kernel == DIINN_DECODE_KERNEL_LATENCY16)
        return launch_sin(sin_mode, [&](auto S) {
            hipLaunchKernelGGL(decode_coop16_kernel<decltype(S)::value>, ch.grid, dim3(256), 0, (hipStream_t)stream, p);
        });
    return launch_sin(sin_mode, [&](auto S) {
        hipLaunchKernelGGL(decode_kernel<decltype(S)::value>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

static int decode_band_impl(void* stream, const float* P_dev, const float* packed_dev,
                            float* out_dev, int B, int H, int W, int Hu, int Wu,
                            int y0, int y1, int sin_mode, int compute, RowWin pw, RowWin ow, bool x3q = false) {
    if (Wu <= 0) return DIINN_ERR_INVALID_ARG;
    return decode_tile_impl(stream, P_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, 0, Wu, sin_mode, compute, pw,
                            contig(ow, Wu), x3q);
}

static int decode_impl(void* stream, const float* feat_dev, const float* packed_dev,
                       float* workspace_dev, float* out_dev,
                       int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode, int compute,
                       RowWin fw, RowWin pw, RowWin ow, bool x3q = false) {
    if (!workspace_dev) return DIINN_ERR_INVALID_ARG;

    int r0, r1;
    int st = diinn_lr_rows_for_band(H, Hu, Wu, y0, y1, &r0, &r1);
    if (st) return st;
    if (!compute_ok(compute))
        return DIINN_ERR_UNSUPPORTED;
    st = launch_P(stream, feat_dev, packed_dev, workspace_dev, B, H, W, r0, r1, 16, p_arith(compute),
                  &fw, &pw, true);
    if (st) return st;
    if (compute == DIINN_COMPUTE_F32_QONLY) {                   // modes 1 and 2: per-cell modulation chain
        st = cell_chain_impl(stream, workspace_dev, packed_dev, B, H, W, r0, r1, pw);
        if (st) return st;
    }
    return decode_band_impl(stream, workspace_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                            compute, pw, ow, x3q);
}

// ---------------------------------------------------------------------------------
// head3x3_reflect_kernel (decoder mode 4, diinn.py:89-90,146: the second half of the 3x3 'reflect' head):
//   out[b, c, y, x] = bL[c] + sum_{k = 0..8} T[b, refl(y + ky - 1, Hu), refl(x + kx - 1, Wu)][k][c],   k = 3 ky + kx,
//   refl(-1, n) = 1, refl(n, n) = n - 2 (PyTorch 'reflect': needs n >= 2).
// One thread per HR pixel, the nine taps added in the fixed order k = 0..8 starting from the bias: deterministic, and a band is
// bit-identical to the same rows of a whole-image decode.  Reflection is applied to IMAGE coordinates; the tap buffer holds rows
// [ty0, ty0 + trows) = [max(0, y0 - 1), min(Hu, y1 + 1)), which contain every reflected row of the band (row -1 -> 1, Hu -> Hu - 2).
// Neighbouring threads read neighbouring 112-byte pixel records: every line of the tap buffer is used whole.  Both validity
// words (the body image's derived sections, the head image's own) are folded into the bias, so a wrong image answers NaN.
// ---------------------------------------------------------------------------------
struct Head3Params {
    const float* taps;     // [B][trows][Wu][TAP_STRIDE]
    const float* Wt;       // body image (validity word only)
    const float* head3;    // head image (bias, validity word)
    float* out;            // [B,3,Orows,Wu] = HR rows [Orow0, Orow0 + Orows)
    int Hu, Wu, y0, y1, ty0, trows, Orow0, Orows;
};
constexpr int H3_BLOCK_W = 64, H3_BLOCK_H = 4;

__global__ __launch_bounds__(256) void head3x3_reflect_kernel(const Head3Params p) {
    const int x = blockIdx.x * H3_BLOCK_W + (threadIdx.x & (H3_BLOCK_W - 1));
    const int y = p.y0 + blockIdx.y * H3_BLOCK_H + (threadIdx.x / H3_BLOCK_W);
    const int b = blockIdx.z;
    if (x >= p.Wu || y >= p.y1) return;
    const unsigned nanm = derived_nan_mask(p.Wt) |
        (__builtin_bit_cast(unsigned, p.head3[HEAD3_BIAS + 3]) == DIINN_HEAD3X3_MAGIC ? 0u : 0x7fc00000u);
    float a0 = or_bits(p.head3[HEAD3_BIAS + 0], nanm);
    float a1 = or_bits(p.head3[HEAD3_BIAS + 1], nanm);
    float a2 = or_bits(p.head3[HEAD3_BIAS + 2], nanm);
    const float* __restrict__ tb = p.taps + (size_t)b * p.trows * p.Wu * TAP_STRIDE;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        int yy = y + ky - 1;
        yy = yy < 0 ? 1 : (yy >= p.Hu ? p.Hu - 2 : yy);
        const float* __restrict__ row = tb + (size_t)(yy - p.ty0) * p.Wu * TAP_STRIDE;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            int xx = x + kx - 1;
            xx = xx < 0 ? 1 : (xx >= p.Wu ? p.Wu - 2 : xx);
            const float* __restrict__ t = row + (size_t)xx * TAP_STRIDE + 3 * (3 * ky + kx);
            a0 += t[0];
            a1 += t[1];
            a2 += t[2];
        }
    }
    const size_t plane = (size_t)p.Orows * p.Wu;
    float* o = p.out + (size_t)b * 3 * plane + (size_t)(y - p.Orow0) * p.Wu + x;
    o[0] = a0;
    o[plane] = a1;
    o[2 * plane] = a2;
}

// Mode 4, HR rows [y0,y1) of the image: the tap form over the extended rows [ty0,ty1) into the tap buffer, then the gather.
// `ow`: the rows `out_dev` holds.  `pw`: the LR rows P_dev holds -- or NULL: P_dev is init_q's pixel planes of exactly the tap
// rows (decode_kernel<SIN | DECODE_INITQ | DECODE_TAPS>).  From P in fp32: the throughput kernel's tap form (no 16-pixel latency
// twin); x3: the tap form of the split-bf16 kernel, decode_bf16x3_kernel<SIN | X3_TAPS>, in its place (the same tap buffer, the
// same gather).
static int decode_mode4_band_impl(void* stream, const float* P_dev, const float* packed_dev, const float* head_dev,
                                  float* taps_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1,
                                  int sin_mode, const RowWin* pw, RowWin ow, bool x3 = false) {
    if (!all_set(P_dev, packed_dev, head_dev, taps_dev, out_dev)) return DIINN_ERR_INVALID_ARG;
    if (int st = check_dims(B, H, W)) return st;
    int ty0, ty1, r0, r1;
    if (int st = diinn_mode4_rows(H, Hu, Wu, y0, y1, &ty0, &ty1, &r0, &r1)) return st;      // Hu, Wu >= 2 and 0 <= y0 < y1 <= Hu
    if (int st = check_extent(Hu, Wu)) return st;
    const RowWin taprows{ty0, ty1 - ty0};
    if (pw)
        if (int st = check_window(pw->row0, pw->rows, H, r0, r1)) return st;
    if (int st = check_window(ow.row0, ow.rows, Hu, y0, y1)) return st;
    if (int st = check_sin(sin_mode)) return st;
    const dim3 grid = decode_grid(B, ty0, ty1, 0, Wu);
    const dim3 hgrid(grid_blocks(0, Wu, H3_BLOCK_W), grid_blocks(y0, y1, H3_BLOCK_H), B);
    if (int st = check_grid(grid.y, B)) return st;
    if (int st = check_grid(hgrid.y, B)) return st;
    // the tap buffer holds the tap rows; the tap form does not use the output strides
    DecodeParams p = decode_params(P_dev, packed_dev, taps_dev, B, H, W, Hu, Wu, ty0, ty1, 0, Wu, pw ? *pw : taprows,
                                   OutView{taprows.row0, taprows.rows, 0, 0, 0, 0});
    p.head3 = head_dev;
    int st;
    if (x3)                                                     // (from init_q's planes: <SIN | X3_INITQ | X3_TAPS>)
        st = launch_decode_bf16x3_form(stream, p, grid, sin_mode, pw ? X3_TAPS : (X3_INITQ | X3_TAPS));
    else if (pw)
        st = launch_sin(sin_mode, [&](auto S) {
            hipLaunchKernelGGL((decode_kernel<decltype(S)::value, true, false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
        });
    else
        st = launch_sin(sin_mode, [&](auto S) {
            hipLaunchKernelGGL(decode_kernel<decltype(S)::value | DECODE_INITQ | DECODE_TAPS>, grid, dim3(256), 0, (hipStream_t)stream, p);
        });
    if (st) return st;
    const Head3Params hp{taps_dev, packed_dev, head_dev, out_dev, Hu, Wu, y0, y1, ty0, ty1 - ty0, ow.row0, ow.rows};
    hipLaunchKernelGGL(head3x3_reflect_kernel, hgrid, dim3(256), 0, (hipStream_t)stream, hp);
    return hip_status(hipGetLastError());
}

// The gather over a WHOLE image for a tap buffer that did not come from decode_kernel<HEAD3>: the training forward of mode 4
// (diinn_mode4_training.hip: head3x3_taps_from_planes_kernel).  That kernel checks the body image itself and accepts a training
// image (DIINN_PACKED_MAGIC_WPU), which the gather -- an inference kernel -- answers with NaN; the gather reads nothing of the body
// image but its validity word, so here it is pointed at a device constant that holds DIINN_PACKED_MAGIC: its own check is then
// the head image's word alone.  The caller has validated the arguments (Hu, Wu >= 2; B and the row blocks within the grid limits).
__attribute__((visibility("hidden"))) __device__ unsigned gather_body_word = DIINN_PACKED_MAGIC;     // (never written)

__attribute__((visibility("hidden")))
int launch_head3x3_whole(void* stream, const float* taps_dev, const float* head_dev, float* out_dev, int B, int Hu, int Wu) {
    void* word = nullptr;
    const hipError_t e = hipGetSymbolAddress(&word, HIP_SYMBOL(gather_body_word));      // a table lookup: no allocation, no synchronisation
    if (e != hipSuccess) return hip_status(e);
    const float* body = (const float*)word - (OFF_BL + 3);                               // the kernel reads body[OFF_BL + 3] only
    const dim3 hgrid((Wu + H3_BLOCK_W - 1) / H3_BLOCK_W, (Hu + H3_BLOCK_H - 1) / H3_BLOCK_H, B);
    const Head3Params hp{taps_dev, body, head_dev, out_dev, Hu, Wu, 0, Hu, 0, Hu, 0, Hu};
    hipLaunchKernelGGL(head3x3_reflect_kernel, hgrid, dim3(256), 0, (hipStream_t)stream, hp);
    return hip_status(hipGetLastError());
}

// init_q (mode 3): HR rows [y0,y1) from the pixel planes of exactly those rows (diinn_initq_planes) into a contiguous [B,3,Hu,Wu].
// The throughput kernel only (no 16-pixel latency twin).  kpart = false: modes 1/2, the planes hold the per-pixel chain
// (diinn_pixel_chain).  x3: split bf16, decode_bf16x3_kernel<SIN | X3_INITQ> (kpart = false: <SIN | X3_INITQ | X3_QONLY>, the chain
// diinn_pixel_chain_x3's).
static int decode_initq_band_impl(void* stream, const float* pix_dev, const float* packed_dev, float* out_dev,
                                  int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode, bool kpart = true,
                                  bool x3 = false) {
    if (int st = check_band_args(B, H, W, Hu, Wu, y0, y1, sin_mode, pix_dev, packed_dev, out_dev)) return st;
    const dim3 grid = decode_grid(B, y0, y1, 0, Wu);
    if (int st = check_grid(grid.y, B)) return st;
    const DecodeParams p = decode_params(pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, 0, Wu,
                                         RowWin{y0, y1 - y0}, contig(RowWin{0, Hu}, Wu));      // P = the pixel planes: HR rows
    if (x3) return launch_decode_bf16x3_form(stream, p, grid, sin_mode, kpart ? X3_INITQ : (X3_INITQ | X3_QONLY));
    return launch_sin<0, 1>(sin_mode, kpart, [&](auto S, auto K) {
        hipLaunchKernelGGL((decode_kernel<decltype(S)::value | DECODE_INITQ, decltype(K)::value>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

// The "all in order" init_q entry points check everything a later launch would refuse BEFORE the first launch, so that a bad
// argument launches nothing: the band checks, then the grid of every launch over HR rows [y0,y1) (row tiles of 8 all).
template <class... T>
static int initq_args_ok(int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode, const T*... ptrs) {
    if (int st = check_band_args(B, H, W, Hu, Wu, y0, y1, sin_mode, ptrs...)) return st;
    return check_grid(grid_blocks(y0, y1, WG_H), B);
}

static int decode_initq_mode12(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                               float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode,
                               bool rows512) {
    int st = initq_args_ok(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, initq_dev, pix_dev, out_dev);
    if (st) return st;
    if ((((size_t)pix_dev) | ((size_t)packed_dev)) & 15) return DIINN_ERR_INVALID_ARG;
    st = launch_initq_planes(stream, feat_dev, packed_dev, initq_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false, rows512);
    if (st) return st;
    st = pixel_chain_impl(stream, pix_dev, packed_dev, B, Wu, y1 - y0, rows512);
    if (st) return st;
    return decode_initq_band_impl(stream, pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false);
}

// The same in split-bf16 arithmetic: initq_planes_x3_kernel (rows512: its 512-row form), pixel_chain_x3_kernel, then
// decode_bf16x3_kernel<SIN | X3_INITQ | X3_QONLY>.  Every check before the first launch.
static int decode_initq_mode12_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                  const float* initq_x3_dev, float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu,
                                  int y0, int y1, int sin_mode, bool rows512) {
    int st = initq_args_ok(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, out_dev);
    if (st) return st;
    if ((((size_t)pix_dev) | ((size_t)packed_dev) | ((size_t)initq_dev) | ((size_t)initq_x3_dev)) & 15) return DIINN_ERR_INVALID_ARG;
    st = launch_initq_planes_x3(stream, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false, rows512);
    if (st) return st;
    st = launch_pixel_chain_x3(stream, pix_dev, packed_dev, B, Wu, y1 - y0, rows512);
    if (st) return st;
    return decode_initq_band_impl(stream, pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false, true);
}

// The training forward's checks after the pointers (its own order: the sine mode before the extent); npix = B Hu Wu
static int check_train_args(int B, int H, int W, int Hu, int Wu, int sin_mode, long long* npix) {
    if (int st = check_dims(B, H, W)) return st;
    if (Hu <= 0 || Wu <= 0) return DIINN_ERR_INVALID_ARG;
    if (int st = check_sin(sin_mode)) return st;
    if (int st = check_extent(Hu, Wu)) return st;
    *npix = (long long)B * Hu * Wu;
    return check_npix(*npix);
}

// The training forward's per-pixel layers over the whole image, one workgroup per four plane tiles: P_dev holds rows `pw` -- the
// hoisted conv (or, kpart = false, the per-cell chain) of all H LR rows, or (initq) the pixel planes of all Hu HR rows, in
// radians.  split_dev (mode 3, from P or from init_q's planes): the split training image -- decode_bf16x3_kernel<SIN | X3_SAVE>, or
// with initq <SIN | X3_INITQ | X3_SAVE>, runs the layers.
static int train_fwd_launch(void* stream, const float* P_dev, const float* packed_dev, float* out_dev, float* acts_dev,
                            int B, int H, int W, int Hu, int Wu, long long npix, int sin_mode, RowWin pw, bool initq, bool kpart,
                            const float* split_dev = nullptr) {
    const dim3 grid((unsigned)((npix + 4 * PLANE_TILE - 1) / (4 * PLANE_TILE)));
    DecodeParams p = decode_params(P_dev, packed_dev, out_dev, B, H, W, Hu, Wu, 0, Hu, 0, Wu, pw, contig(RowWin{0, Hu}, Wu));
    p.acts = acts_dev; p.npix = npix;
    if (split_dev) {
        p.split = split_dev;
        return launch_decode_bf16x3_form(stream, p, grid, sin_mode, initq ? (X3_INITQ | X3_SAVE) : X3_SAVE);
    }
    int st = DIINN_ERR_UNSUPPORTED;
    pick<0, DECODE_INITQ>(initq ? DECODE_INITQ : 0, [&](auto Q) {
        st = launch_sin<0, 1>(sin_mode, kpart, [&](auto S, auto K) {
            hipLaunchKernelGGL((decode_kernel<decltype(S)::value | decltype(Q)::value, decltype(K)::value, true>), grid, dim3(256), 0,
                               (hipStream_t)stream, p);
        });
    });
    return st;
}

// The training forward, KPART = true (mode 3) or false (modes 1/2: P_dev holds the per-cell chain, diinn_cell_chain)
static int train_fwd_impl(void* stream, const float* P_dev, const float* packed_dev, float* out_dev,
                          float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode, bool kpart,
                          const float* split_dev = nullptr) {
    if (!all_set(P_dev, packed_dev, out_dev, acts_dev)) return DIINN_ERR_INVALID_ARG;
    long long npix;
    if (int st = check_train_args(B, H, W, Hu, Wu, sin_mode, &npix)) return st;
    return train_fwd_launch(stream, P_dev, packed_dev, out_dev, acts_dev, B, H, W, Hu, Wu, npix, sin_mode, RowWin{0, H}, false, kpart,
                            split_dev);
}

// init_q (mode 3) under autograd: the pixel planes of the WHOLE image in radians (initq_planes_kernel<SIN | INITQ_RAD> on the init_q
// training image), then decode_kernel<SIN | DECODE_INITQ, true, SAVE>: acts in diinn_decode_train_fwd's layout, s_0 in radians.
// chain: 0 = mode 3; 1 / 2 = modes 1/2 (pixel_chain_kernel over all Hu rows between the planes and the layers, KPART = false),
// 2 with the chain's layers 1..3 seeded from bK_i of the body image (diinn_pixel_chain's bk_seeds)
static int initq_train_fwd_impl(void* stream, const float* feat_dev, const float* packed_dev, const float* train_image_dev,
                                float* pix_dev, float* out_dev, float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode,
                                int chain) {
    if (!all_set(feat_dev, packed_dev, train_image_dev, pix_dev, out_dev, acts_dev)) return DIINN_ERR_INVALID_ARG;
    long long npix;
    int st = check_train_args(B, H, W, Hu, Wu, sin_mode, &npix);
    if (st) return st;
    if ((((size_t)packed_dev) | ((size_t)train_image_dev) | ((size_t)pix_dev)) & 15) return DIINN_ERR_INVALID_ARG;   // 16-byte pieces and seeds
    // (what the two launches in front of decode_kernel would refuse: checked before the first of them)
    st = check_grid(grid_blocks(0, Hu, WG_H), B);
    if (st) return st;
    st = launch_initq_planes(stream, feat_dev, packed_dev, train_image_dev, pix_dev, B, H, W, Hu, Wu, 0, Hu, sin_mode, true);
    if (st) return st;
    if (chain) {
        st = pixel_chain_impl(stream, pix_dev, packed_dev, B, Wu, Hu, chain == 2);
        if (st) return st;
    }
    return train_fwd_launch(stream, pix_dev, packed_dev, out_dev, acts_dev, B, H, W, Hu, Wu, npix, sin_mode, RowWin{0, Hu}, true,
                            chain == 0);
}

// The same in split-bf16 arithmetic (mode 3): initq_planes_x3_kernel<SIN | INITQ_X3_RAD> on the init_q training image and the init_q
// split training image, then decode_bf16x3_kernel<SIN | X3_INITQ | X3_SAVE> on the split training image of the body image.
static int initq_train_fwd_x3_impl(void* stream, const float* feat_dev, const float* packed_dev, const float* train_image_dev,
                                   const float* split_dev, const float* initq_split_dev, float* pix_dev, float* out_dev,
                                   float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode) {
    if (!all_set(feat_dev, packed_dev, train_image_dev, split_dev, initq_split_dev, pix_dev, out_dev, acts_dev)) return DIINN_ERR_INVALID_ARG;
    long long npix;
    int st = check_train_args(B, H, W, Hu, Wu, sin_mode, &npix);
    if (st) return st;
    if ((((size_t)packed_dev) | ((size_t)train_image_dev) | ((size_t)split_dev) | ((size_t)initq_split_dev) | ((size_t)pix_dev)) & 15)
        return DIINN_ERR_INVALID_ARG;                               // 16-byte pieces and seeds
    st = check_grid(grid_blocks(0, Hu, WG_H), B);
    if (st) return st;
    st = launch_initq_planes_x3(stream, feat_dev, packed_dev, train_image_dev, initq_split_dev, pix_dev, B, H, W, Hu, Wu, 0, Hu, sin_mode, true);
    if (st) return st;
    return train_fwd_launch(stream, pix_dev, packed_dev, out_dev, acts_dev, B, H, W, Hu, Wu, npix, sin_mode, RowWin{0, Hu}, true, true,
                            split_dev);
}

extern "C" {

int diinn_pixel_chain(void* stream, float* pix_dev, const float* packed_dev, int B, int Wu, int rows, int bk_seeds) {
    return pixel_chain_impl(stream, pix_dev, packed_dev, B, Wu, rows, bk_seeds != 0);
}

int diinn_decode_initq_qonly_band(void* stream, const float* pix_dev, const float* packed_dev, float* out_dev,
                                  int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return decode_initq_band_impl(stream, pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false);
}

int diinn_decode_initq_mode1(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                             float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return decode_initq_mode12(stream, feat_dev, packed_dev, initq_dev, pix_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, true);
}

int diinn_decode_initq_mode2(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                             float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return decode_initq_mode12(stream, feat_dev, packed_dev, initq_dev, pix_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false);
}

// init_q with mode 4: the pixel planes hold the tap rows [ty0,ty1) = [max(0, y0-1), min(Hu, y1+1)); out_dev is a contiguous [B,3,Hu,Wu]
int diinn_decode_initq_mode4_band(void* stream, const float* pix_dev, const float* packed_dev, const float* head_dev,
                                  float* taps_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1,
                                  int sin_mode) {
    return decode_mode4_band_impl(stream, pix_dev, packed_dev, head_dev, taps_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                                  nullptr, RowWin{0, Hu});
}

int diinn_decode_initq_mode4(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                             const float* head_dev, float* pix_dev, float* taps_dev, float* out_dev,
                             int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    if (!all_set(head_dev, taps_dev)) return DIINN_ERR_INVALID_ARG;
    int st = initq_args_ok(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, initq_dev, pix_dev, out_dev);
    if (st) return st;
    int ty0, ty1, r0, r1;
    st = diinn_mode4_rows(H, Hu, Wu, y0, y1, &ty0, &ty1, &r0, &r1);
    if (st) return st;
    st = check_grid(grid_blocks(ty0, ty1, WG_H), B);
    if (st) return st;
    st = diinn_initq_planes(stream, feat_dev, packed_dev, initq_dev, pix_dev, B, H, W, Hu, Wu, ty0, ty1, sin_mode);
    if (st) return st;
    return diinn_decode_initq_mode4_band(stream, pix_dev, packed_dev, head_dev, taps_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode);
}

// init_q with modes 1, 2 and 4 in split-bf16 arithmetic (behind ImplicitDecoder.hip_initq_modes_split_bf16): the arguments of the fp32
// twins plus the init_q split image
int diinn_decode_initq_mode1_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                const float* initq_x3_dev, float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu,
                                int y0, int y1, int sin_mode) {
    return decode_initq_mode12_x3(stream, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, true);
}

int diinn_decode_initq_mode2_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                const float* initq_x3_dev, float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu,
                                int y0, int y1, int sin_mode) {
    return decode_initq_mode12_x3(stream, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, false);
}

// planes of the tap rows (initq_planes_x3_kernel), decode_bf16x3_kernel<SIN | X3_INITQ | X3_TAPS>, head3x3_reflect_kernel unchanged
int diinn_decode_initq_mode4_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                                const float* initq_x3_dev, const float* head_dev, float* pix_dev, float* taps_dev, float* out_dev,
                                int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    if (!all_set(head_dev, taps_dev)) return DIINN_ERR_INVALID_ARG;
    int st = initq_args_ok(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, out_dev);
    if (st) return st;
    if ((((size_t)pix_dev) | ((size_t)packed_dev) | ((size_t)initq_dev) | ((size_t)initq_x3_dev) | ((size_t)head_dev)) & 15)
        return DIINN_ERR_INVALID_ARG;
    int ty0, ty1, r0, r1;
    st = diinn_mode4_rows(H, Hu, Wu, y0, y1, &ty0, &ty1, &r0, &r1);
    if (st) return st;
    st = check_grid(grid_blocks(ty0, ty1, WG_H), B);
    if (st) return st;
    st = launch_initq_planes_x3(stream, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, B, H, W, Hu, Wu, ty0, ty1, sin_mode);
    if (st) return st;
    return decode_mode4_band_impl(stream, pix_dev, packed_dev, head_dev, taps_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                                  nullptr, RowWin{0, Hu}, true);
}

int diinn_decode_initq_band(void* stream, const float* pix_dev, const float* packed_dev, float* out_dev,
                            int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return decode_initq_band_impl(stream, pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode);
}

// init_q (mode 3) in split-bf16 arithmetic: initq_planes_x3_kernel, decode_bf16x3_kernel<SIN | X3_INITQ>
int diinn_decode_initq_band_x3(void* stream, const float* pix_dev, const float* packed_dev, float* out_dev,
                               int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return decode_initq_band_impl(stream, pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, true, true);
}

int diinn_decode_initq_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                          const float* initq_x3_dev, float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu,
                          int y0, int y1, int sin_mode) {
    if (!out_dev) return DIINN_ERR_INVALID_ARG;
    const int st = diinn_initq_planes_x3(stream, feat_dev, packed_dev, initq_dev, initq_x3_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode);
    if (st) return st;
    return decode_initq_band_impl(stream, pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, true, true);
}

int diinn_decode_initq(void* stream, const float* feat_dev, const float* packed_dev, const float* initq_dev,
                       float* pix_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    if (!out_dev) return DIINN_ERR_INVALID_ARG;
    const int st = diinn_initq_planes(stream, feat_dev, packed_dev, initq_dev, pix_dev, B, H, W, Hu, Wu, y0, y1, sin_mode);
    if (st) return st;
    return decode_initq_band_impl(stream, pix_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode);
}

int diinn_decode_mode4_band(void* stream, const float* P_dev, const float* packed_dev, const float* head_dev,
                            float* taps_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1,
                            int sin_mode) {
    const RowWin full{0, H};
    return decode_mode4_band_impl(stream, P_dev, packed_dev, head_dev, taps_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                                  &full, RowWin{0, Hu});
}

int diinn_decode_mode4(void* stream, const float* feat_dev, const float* packed_dev, const float* head_dev,
                       float* workspace_dev, float* taps_dev, float* out_dev,
                       int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    if (!all_set(workspace_dev, head_dev, taps_dev, out_dev)) return DIINN_ERR_INVALID_ARG;
    int ty0, ty1, r0, r1;
    int st = diinn_mode4_rows(H, Hu, Wu, y0, y1, &ty0, &ty1, &r0, &r1);
    if (st) return st;
    st = check_sin(sin_mode);
    if (st) return st;
    const RowWin full{0, H};
    st = launch_P(stream, feat_dev, packed_dev, workspace_dev, B, H, W, r0, r1, 16, 0, &full, &full, true);
    if (st) return st;
    return decode_mode4_band_impl(stream, workspace_dev, packed_dev, head_dev, taps_dev, out_dev, B, H, W, Hu, Wu, y0, y1,
                                  sin_mode, &full, RowWin{0, Hu});
}

// ---- decoder modes 1, 2 and 4 in split-bf16 arithmetic (include/diinn_hip.h; opt-in: ImplicitDecoder.hip_modes_split_bf16) ----
// (what every launch of these entry points would refuse is checked before the first of them: check_band_args, then the grids)
int diinn_decode_qonly_x3_band(void* stream, const float* P_dev, const float* packed_dev, float* out_dev,
                               int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return decode_band_impl(stream, P_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, DIINN_COMPUTE_F32_QONLY,
                            RowWin{0, H}, RowWin{0, Hu}, true);
}

int diinn_decode_qonly_x3(void* stream, const float* feat_dev, const float* packed_dev, float* workspace_dev, float* out_dev,
                          int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    int st = check_band_args(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, workspace_dev, out_dev);
    if (st) return st;
    st = check_grid(grid_blocks(y0, y1, WG_H), B);
    if (st) return st;
    // P and the per-cell chain in fp32 (DIINN_COMPUTE_F32_QONLY's), the per-pixel layers on decode_bf16x3_kernel<SIN | X3_QONLY>
    return decode_impl(stream, feat_dev, packed_dev, workspace_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                       DIINN_COMPUTE_F32_QONLY, RowWin{0, H}, RowWin{0, H}, RowWin{0, Hu}, true);
}

int diinn_decode_mode4_x3_band(void* stream, const float* P_dev, const float* packed_dev, const float* head_dev,
                               float* taps_dev, float* out_dev, int B, int H, int W, int Hu, int Wu, int y0, int y1,
                               int sin_mode) {
    const RowWin full{0, H};
    return decode_mode4_band_impl(stream, P_dev, packed_dev, head_dev, taps_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                                  &full, RowWin{0, Hu}, true);
}

int diinn_decode_mode4_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* head_dev,
                          float* workspace_dev, float* taps_dev, float* out_dev,
                          int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    if (!all_set(head_dev, taps_dev)) return DIINN_ERR_INVALID_ARG;
    int st = check_band_args(B, H, W, Hu, Wu, y0, y1, sin_mode, feat_dev, packed_dev, workspace_dev, out_dev);
    if (st) return st;
    int ty0, ty1, r0, r1;
    st = diinn_mode4_rows(H, Hu, Wu, y0, y1, &ty0, &ty1, &r0, &r1);
    if (st) return st;
    st = check_grid(grid_blocks(ty0, ty1, WG_H), B);
    if (st) return st;
    st = check_grid(grid_blocks(y0, y1, H3_BLOCK_H), B);
    if (st) return st;
    const RowWin full{0, H};
    // the hoisted conv as DIINN_COMPUTE_BF16X3 runs it for mode 3 (split bf16 on large maps, the fp32 Winograd form below)
    st = launch_P(stream, feat_dev, packed_dev, workspace_dev, B, H, W, r0, r1, 16, p_arith(DIINN_COMPUTE_BF16X3), &full, &full, true);
    if (st) return st;
    return decode_mode4_band_impl(stream, workspace_dev, packed_dev, head_dev, taps_dev, out_dev, B, H, W, Hu, Wu, y0, y1,
                                  sin_mode, &full, RowWin{0, Hu}, true);
}

int diinn_cell_chain(void* stream, float* P_dev, const float* packed_dev, int B, int H, int W, int r0, int r1) {
    return cell_chain_impl(stream, P_dev, packed_dev, B, H, W, r0, r1, RowWin{0, H});
}

int diinn_decode_launch_info(int B, int Hu, int Wu, int y0, int y1,
                             int* grid_x, int* grid_y, int* grid_z, int* block) {
    if (B <= 0 || check_band(Hu, Wu, y0, y1)) return DIINN_ERR_INVALID_ARG;
    const dim3 grid = decode_grid(B, y0, y1, 0, Wu);
    if (grid_x) *grid_x = (int)grid.x;
    if (grid_y) *grid_y = (int)grid.y;
    if (grid_z) *grid_z = (int)grid.z;
    if (block) *block = 256;
    return DIINN_OK;
}

int diinn_decode_kernel_info(int B, int Hu, int Wu, int y0, int y1, int x0, int x1, int compute, int info[4]) {
    if (!info || B <= 0 || check_band(Hu, Wu, y0, y1) || x0 < 0 || x1 > Wu || x0 >= x1) return DIINN_ERR_INVALID_ARG;
    if (!compute_ok(compute)) return DIINN_ERR_UNSUPPORTED;
    F32Choice ch{compute == DIINN_COMPUTE_F32_QONLY ? DIINN_DECODE_KERNEL_THROUGHPUT : DIINN_DECODE_KERNEL_OTHER,
                 decode_grid(B, y0, y1, x0, x1)};
    if (compute == DIINN_COMPUTE_F32) ch = f32_kernel_choice(B, y0, y1, x0, x1);
    info[0] = ch.kernel; info[1] = (int)ch.grid.x; info[2] = (int)ch.grid.y; info[3] = (int)ch.grid.z;
    return DIINN_OK;
}

int diinn_decode_band(void* stream, const float* P_dev, const float* packed_dev,
                      float* out_dev, int B, int H, int W, int Hu, int Wu,
                      int y0, int y1, int sin_mode) {
    return diinn_decode_band_ex(stream, P_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                                DIINN_COMPUTE_F32);
}

int diinn_decode_band_ex(void* stream, const float* P_dev, const float* packed_dev,
                         float* out_dev, int B, int H, int W, int Hu, int Wu,
                         int y0, int y1, int sin_mode, int compute) {
    return decode_band_impl(stream, P_dev, packed_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, compute,
                            RowWin{0, H}, RowWin{0, Hu});
}

int diinn_decode_band_win(void* stream, const float* P_win_dev, int p_row0, int p_rows, const float* packed_dev,
                          float* out_win_dev, int out_row0, int out_rows,
                          int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode, int compute) {
    return decode_band_impl(stream, P_win_dev, packed_dev, out_win_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, compute,
                            RowWin{p_row0, p_rows}, RowWin{out_row0, out_rows});
}

int diinn_decode_tile_win(void* stream, const float* P_win_dev, int p_row0, int p_rows, const float* packed_dev,
                          float* out_tile_dev, long long out_row_stride, long long out_plane_stride,
                          long long out_batch_stride, int B, int H, int W, int Hu, int Wu,
                          int y0, int y1, int x0, int x1, int sin_mode, int compute) {
    // the view starts at the tile's own first pixel: row0 = y0, col0 = x0, rows = what the tile covers
    return decode_tile_impl(stream, P_win_dev, packed_dev, out_tile_dev, B, H, W, Hu, Wu, y0, y1, x0, x1, sin_mode, compute,
                            RowWin{p_row0, p_rows},
                            OutView{y0, y1 > y0 ? y1 - y0 : 1, x0, out_batch_stride, out_plane_stride, out_row_stride});
}

int diinn_decode_train_fwd(void* stream, const float* P_dev, const float* packed_dev, float* out_dev,
                           float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode) {
    return train_fwd_impl(stream, P_dev, packed_dev, out_dev, acts_dev, B, H, W, Hu, Wu, sin_mode, true);
}

int diinn_decode_train_fwd_x3(void* stream, const float* P_dev, const float* packed_dev, const float* split_dev, float* out_dev,
                              float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode) {
    if (!split_dev || (((size_t)split_dev) & 15)) return DIINN_ERR_INVALID_ARG;     // 16-byte weight pieces
    return train_fwd_impl(stream, P_dev, packed_dev, out_dev, acts_dev, B, H, W, Hu, Wu, sin_mode, true, split_dev);
}

int diinn_decode_initq_train_fwd(void* stream, const float* feat_dev, const float* packed_dev, const float* train_image_dev,
                                 float* pix_dev, float* out_dev, float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode) {
    return initq_train_fwd_impl(stream, feat_dev, packed_dev, train_image_dev, pix_dev, out_dev, acts_dev, B, H, W, Hu, Wu, sin_mode, 0);
}

int diinn_decode_initq_train_fwd_x3(void* stream, const float* feat_dev, const float* packed_dev, const float* train_image_dev,
                                    const float* split_dev, const float* initq_split_dev, float* pix_dev, float* out_dev,
                                    float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode) {
    return initq_train_fwd_x3_impl(stream, feat_dev, packed_dev, train_image_dev, split_dev, initq_split_dev, pix_dev, out_dev, acts_dev,
                                   B, H, W, Hu, Wu, sin_mode);
}

// init_q with modes 1/2 under autograd: the radians planes of the whole image, pixel_chain_kernel over all Hu rows, then
// decode_kernel<SIN | DECODE_INITQ, false, SAVE>: k_i as the chain left it in the pixel record, s_i in radians.
int diinn_decode_initq_train_fwd_qonly(void* stream, const float* feat_dev, const float* packed_dev, const float* train_image_dev,
                                       float* pix_dev, float* out_dev, float* acts_dev, int B, int H, int W, int Hu, int Wu,
                                       int sin_mode, int bk_seeds) {
    return initq_train_fwd_impl(stream, feat_dev, packed_dev, train_image_dev, pix_dev, out_dev, acts_dev, B, H, W, Hu, Wu, sin_mode,
                                bk_seeds ? 2 : 1);
}

int diinn_decode_train_fwd_qonly(void* stream, const float* chain_dev, const float* packed_dev, float* out_dev,
                                 float* acts_dev, int B, int H, int W, int Hu, int Wu, int sin_mode) {
    return train_fwd_impl(stream, chain_dev, packed_dev, out_dev, acts_dev, B, H, W, Hu, Wu, sin_mode, false);
}

int diinn_decode(void* stream, const float* feat_dev, const float* packed_dev,
                 float* workspace_dev, float* out_dev,
                 int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode) {
    return diinn_decode_ex(stream, feat_dev, packed_dev, workspace_dev, out_dev, B, H, W, Hu, Wu, y0, y1,
                           sin_mode, DIINN_COMPUTE_F32);
}

int diinn_decode_ex(void* stream, const float* feat_dev, const float* packed_dev,
                    float* workspace_dev, float* out_dev,
                    int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode, int compute) {
    return decode_impl(stream, feat_dev, packed_dev, workspace_dev, out_dev, B, H, W, Hu, Wu, y0, y1, sin_mode, compute,
                       RowWin{0, H}, RowWin{0, H}, RowWin{0, Hu});
}

int diinn_decode_win(void* stream, const float* feat_win_dev, int feat_row0, int feat_rows,
                     const float* packed_dev, float* P_win_dev, int p_row0, int p_rows,
                     float* out_win_dev, int out_row0, int out_rows,
                     int B, int H, int W, int Hu, int Wu, int y0, int y1, int sin_mode, int compute) {
    return decode_impl(stream, feat_win_dev, packed_dev, P_win_dev, out_win_dev, B, H, W, Hu, Wu, y0, y1, sin_mode,
                       compute, RowWin{feat_row0, feat_rows}, RowWin{p_row0, p_rows}, RowWin{out_row0, out_rows});
}

}  // extern "C"
