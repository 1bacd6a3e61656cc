// unit1_c64.hip — the stem and the whole FIRST residual unit of the IR-ResNet (stage 1, unit 1) in ONE rolling-row launch:
//
//     s = PReLU(stem(pixels))                          112 x 112 x 64      (front_c64.hip / stem_kernel)
//     t = PReLU(conv1(s) + b1[border class])           112 x 112 x 64      (front_c64.hip)
//     y = conv2_stride2(t) + shortcut_1x1_stride2(s) + b                   56 x 56 x 64   (conv3x3_s2c64.hip, SC form)
//
// As two launches (front_c64 + conv3x3_s2c64) t is written to HBM once and read once, 2 x 469 MB per 292 images, and the
// quarter of s the shortcut samples makes the same trip (2 x 117 MB): 1.17 GB that nothing else reads in the inference
// forward.  Here only the pixels come in and y goes out:
//
//   * one persistent 8-wave workgroup per CU owns a contiguous range of OUTPUT rows of the batch seen as one tall image
//     (N * 56 rows) and rolls through image boundaries.  A PASS is one input row (112 pixels = seven whole MFMA tiles);
//     an output row is finished every second pass;
//   * waves 0..3 compute conv1: each holds the weights of 32 output channels in registers (144 VGPRs) and does four or
//     three of the row's seven tiles.  Waves 4..7 park the pixel row, compute the stem row (two channel tiles x three or
//     four pixel tiles each, so that every SIMD sees seven) and, every second pass, one output row of conv2 + shortcut for
//     16 output channels each (80 weight registers).  Waves w and w + 4 share a SIMD;
//   * three rings in LDS, each filled by computation: 4 pixel-record rows (front_c64.hip's 32-byte records), 5 stem rows
//     (three for conv1, and the row the shortcut samples lives four passes), 4 t rows written by conv1's epilogue
//     DE-INTERLEAVED into an odd and an even plane — the layout conv3x3_s2c64.hip creates on the way in — so that every tap of
//     the stride-2 convolution reads 16 consecutive positions.  The shortcut reads the odd positions of its stem row in place;
//   * ONE barrier per pass.  In pass k: pixel row G - 3 + k is parked, stem row G - 5 + k, t row G - 7 + k and (k odd)
//     output row (G - 9 + k) / 2 are computed (G = twice the range's first output row), each from what the passes before
//     left.  Rows above and below an image are read from one zero row (a wave-uniform choice of the row's base address).
//
// Bit-identical to the two launches: the same packed weights and lane permutation, the stem's two K-steps with the bias as
// start value, conv1's (tap, K half) walk and epilogue, conv2's nine taps x two K halves followed by the shortcut's two
// K-steps, and rounding to 16 bits at the same three places.  (The sums of an output element do not depend on which wave
// holds its channel.)  Stores are ordinary predicated stores (front_c64.hip on what raced otherwise).
// Reference: insightface fresnet conv0/bn0/relu0 + stage1_unit1, executed inside model.forward at
// /root/reference/code/face_model.py:90.
#include "conv_device.h"

namespace alink {
namespace {

typedef __attribute__((__vector_size__(4 * sizeof(int)))) int i32x4;
typedef __attribute__((__vector_size__(2 * sizeof(int)))) int i32x2;

// every LDS operation of this wave has completed (the rows it wrote, the operand reads of the pass before), then the
// workgroup barrier.  No vector-memory wait: pixels land in registers (the compiler waits where they are used) and the
// output stores may stay in flight.
__device__ __forceinline__ void lds_done_then_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int A>
struct IC { static constexpr int a = A; };

constexpr int NT = 512;
constexpr int W = 112, H = 112, WO = 56, HO = 56;
constexpr int SPITCH = (W + 2) * 128;           // a stem row slot: zero pixel, W pixels, zero pixel
constexpr int SR = 5;                           // stem row slots
constexpr int ODDB = (WO + 1) * 128;            // a t row slot: the odd pixels behind a zero pixel, then the even pixels
constexpr int TPITCH = ODDB + WO * 128;
constexpr int TR = 4;                           // t row slots
constexpr int IMPX = 32;                        // a pixel's record: its 3 x 3-channel window of the row (9 values) + 7 zeros
constexpr int IMROWB = W * IMPX;
constexpr int IR = 4;                           // pixel-record rows
// The half-empty fourth tile of an output row reads up to 8 positions past its plane and the shortcut up to 14 past its
// stem row (values the dead MFMA columns ignore): every region below is followed by at least that much LDS.
constexpr int TOFF = 0;
constexpr int SOFF = TOFF + TR * TPITCH;
constexpr int ZOFF = SOFF + SR * SPITCH;        // one zero row: stands in for a stem row, a t row or a pixel-record row outside the image
constexpr int IOFF = ZOFF + SPITCH;
constexpr int BOFF = IOFF + IR * IMROWB;        // tables: conv1's bias classes [9][64] + slopes, the stem's slopes, conv2's bias
constexpr int TBYTES = 12 * 64 * 4;
constexpr int SINKOFF = BOFF + TBYTES;          // 16 B nobody reads
constexpr size_t LDS_BYTES = (size_t)SINKOFF + 16;
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
static_assert(ZOFF + ODDB + 64 * 128 <= (int)LDS_BYTES && SOFF + (SR - 1) * SPITCH + 128 * 128 <= (int)LDS_BYTES, "operand overrun stays inside LDS");

struct Unit1Params {
    const void*  w1;      // conv1: [64][576] T, rows perm32-permuted
    const float* b1;      // [9][64] by border class
    const float* a1;      // [64] PReLU slopes
    const void*  w2;      // conv2 + shortcut: [64][640] T
    const float* b2;      // [64]
    void*        out;     // [N][56][56][64] T
    StemParams   s;
    int N;
};

template <bool AMAX>
__device__ __forceinline__ float prelu(float v, float slope) {
    const float w = v * slope;
    return AMAX ? __builtin_fmaxf(v, w) : (v > 0.f ? v : w);
}

// ---- waves 0..3: conv1.  HALF 0: the row's tiles 0..3, HALF 1: tiles 4..6 ------------------------------------------------------
template <typename T, bool AMAX, int HALF>
__device__ __forceinline__ void conv1_wave(const Unit1Params& p, char* smem, int ch, int G0, int NP) {
    typedef typename Vec8<T>::type vec8;
    constexpr int NTL = HALF == 0 ? 4 : 3, U0 = HALF == 0 ? 0 : 4;
    const int lane = threadIdx.x & 63, q = lane >> 4, lr = lane & 15;
    const int d = delta(lr);

    const T* __restrict__ gw = (const T*)p.w1;
    vec8 wr[2][9][2];                                  // [channel tile][tap][K half]
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                wr[ct][tap][ks] = *(const vec8*)(gw + (size_t)(ch * 32 + 16 * ct + lr) * 576 + tap * 64 + ks * 32 + 8 * q);
    int loff[3][2];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            loff[kx][ks] = (d + kx) * 128 + ((((ks << 2) | q) ^ (((d + kx) >> 1) & 7)) << 4) + 2048 * U0;
    // where the lane's pixel x = 16 u + d lands in a t slot: plane by parity, position x / 2 (+ 1 behind the zero pixel)
    const int tp0 = (d >> 1) + (d & 1);
    const int tbase = ((d & 1) ? 0 : ODDB) + tp0 * 128;
    const int jp = 4 * ch + q;                         // the lane's 8 channels = one 16-B piece
    const float* const eb1 = (const float*)(smem + BOFF);
    const float* const ea1 = eb1 + 9 * 64;

#pragma unroll 1
    for (int k = 0; k < NP; ++k) {
        lds_done_then_barrier();
        if (k < 6 || k > NP - 2) continue;
        const int r = (G0 - 7 + k + H) % H;            // the t row of this pass (>= -1) in its image
        int sb[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) sb[ky] = SOFF + ((k - 3 + ky) % SR) * SPITCH;
        if (r == 0) sb[0] = ZOFF;
        if (r == H - 1) sb[2] = ZOFF;

        f32x4 acc[2][NTL];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int u = 0; u < NTL; ++u) acc[ct][u] = f32x4{0.f, 0.f, 0.f, 0.f};
        vec8 pf[2][NTL];
#pragma unroll
        for (int u = 0; u < NTL; ++u) pf[0][u] = *(const vec8*)(smem + (sb[0] + loff[0][0]) + 2048 * u);
#pragma unroll
        for (int st = 0; st < 18; ++st) {
            if (st + 1 < 18) {
                const int tn = (st + 1) >> 1, ksn = (st + 1) & 1;
#pragma unroll
                for (int u = 0; u < NTL; ++u)
                    pf[(st + 1) & 1][u] = *(const vec8*)(smem + (sb[tn / 3] + loff[tn % 3][ksn]) + 2048 * u);
            }
            const int tap = st >> 1, ks = st & 1;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int u = 0; u < NTL; ++u) acc[ct][u] = mfma16<T>(wr[ct][tap][ks], pf[st & 1][u], acc[ct][u]);
        }

        // epilogue: folded-BN bias by border class + PReLU, 8 consecutive channels per lane, into the t ring
        const int rc = r == 0 ? 0 : (r == H - 1 ? 2 : 1);
        char* const tslot = smem + TOFF + (k & (TR - 1)) * TPITCH + tbase;
        const f32x4 al0 = *(const f32x4*)(ea1 + ch * 32 + 8 * q), al1 = *(const f32x4*)(ea1 + ch * 32 + 8 * q + 4);
#pragma unroll
        for (int u = 0; u < NTL; ++u) {
            const int x = 16 * (U0 + u) + d;
            const int cls = rc * 3 + (x == 0 ? 0 : (x == W - 1 ? 2 : 1));
            const f32x4 b0 = *(const f32x4*)(eb1 + cls * 64 + ch * 32 + 8 * q);
            const f32x4 b1 = *(const f32x4*)(eb1 + cls * 64 + ch * 32 + 8 * q + 4);
            float v[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = acc[0][u][j] + b0[j]; v[4 + j] = acc[1][u][j] + b1[j]; }
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = prelu<AMAX>(v[i], i < 4 ? al0[i & 3] : al1[i & 3]);
            vec8 o8;
#pragma unroll
            for (int i = 0; i < 8; ++i) o8[i] = (T)v[i];
            const int pos = 8 * (U0 + u) + tp0;        // position in the plane
            *(vec8*)(tslot + 1024 * (U0 + u) + ((jp ^ ((pos >> 1) & 7)) << 4)) = o8;
        }
    }
}

// ---- waves 4..7: pixels, stem, conv2 + shortcut.  b = 0..3; SHALF 0: the stem row's tiles 0..3, SHALF 1: tiles 4..6 ------------
template <typename T, int LAYOUT, bool AMAX, int SHALF>
__device__ __forceinline__ void stem_conv2_wave(const Unit1Params& p, char* smem, int b, int R0, int NP) {
    typedef typename Vec8<T>::type vec8;
    const StemParams& s = p.s;
    const int tb = threadIdx.x - 256, lane = tb & 63, q = lane >> 4, lr = lane & 15;
    const int d = delta(lr);
    const int sch = b & 1;                             // stem: which half of a lane's 16 channels
    const int cch = b >> 1, cct = b & 1;               // conv2: output channels 32 cch + 8 q + 4 cct .. + 3
    const int G0 = 2 * R0;
    const int last_row = p.N * H - 1;                  // (the launcher keeps N * H * W * 64 below 2^31)

    // stem: weight rows 16 t + lr of tiles t = 2 sch, 2 sch + 1 (front_c64.hip); K = 64 in two steps of 32
    vec8 swf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int st = 0; st < 2; ++st) swf[t][st] = *(const vec8*)((const T*)s.wgt + (16 * (2 * sch + t) + lr) * 64 + st * 32 + 8 * q);
    float sbi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sbi[i] = s.bias[16 * q + 8 * sch + i];
    const int rec_off = lr * IMPX + (q & 1) * 16;
    const int sw_off = (lr + 1) * 128 + (((2 * q + sch) ^ (((lr + 1) >> 1) & 7)) << 4);

    // conv2: the wave's 16 output channels x (9 taps + shortcut) x two K halves
    constexpr int KR = 9 * 64 + 64;
    const T* __restrict__ gw2 = (const T*)p.w2 + (size_t)(cch * 32 + 16 * cct + lr) * KR + 8 * q;
    vec8 w2r[9][2], ws[2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) w2r[tap][ks] = *(const vec8*)(gw2 + tap * 64 + ks * 32);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) ws[ks] = *(const vec8*)(gw2 + 9 * 64 + ks * 32);
    int loff2[2][2], scoff[2];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) loff2[e][ks] = (d + e) * 128 + ((((ks << 2) | q) ^ (((d + e) >> 1) & 7)) << 4);
    // the shortcut's operand: stem pixel 2 x, x = 16 t + d, sits at position 2 x + 1 of its slot
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) scoff[ks] = (2 * d + 1) * 128 + ((((ks << 2) | q) ^ (d & 7)) << 4);
    const float* const salpha = (const float*)(smem + BOFF) + 10 * 64;
    const float* const eb2 = salpha + 64;

    // ---- the pixel row: 336 values, up to two per thread of this group (front_c64.hip's load_pair / store_pair for one row)
    int goff[2], soff[2];
    float ssub[2];
    {
        float sb0 = s.sub[0], sb1 = s.sub[1], sb2 = s.sub[2];
        asm volatile("" : "+s"(sb0), "+s"(sb1), "+s"(sb2));
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int i = tb + 256 * jj;
            const bool valid = i < 3 * W;
            const int e = valid ? i : 0;
            int c, ix;
            if (LAYOUT == ALINK_LAYOUT_NCHW_F32) { c = e / W; ix = e - c * W; }
            else                                 { ix = e / 3; c = e - ix * 3; }
            const int cn = s.flip ? 2 - c : c;
            ssub[jj] = cn == 0 ? sb0 : (cn == 1 ? sb1 : sb2);
            goff[jj] = LAYOUT == ALINK_LAYOUT_NCHW_F32 ? c * H * W + ix : e;
            soff[jj] = valid ? (ix + 1) * IMPX + cn * 2 : -1;
        }
    }
    constexpr int ROWP = LAYOUT == ALINK_LAYOUT_NCHW_F32 ? W : W * 3;
    char* const sink = smem + SINKOFF;
    // row g of the batch seen as one tall image, clamped into it (a clamped row is only read by rows nobody uses)
    auto load_row = [&](int g, float (&raw)[2]) __attribute__((always_inline)) {
        g = g < 0 ? 0 : (g > last_row ? last_row : g);
        const int n = g / H, iy = g - n * H;
        const long long base = (long long)n * 3 * H * W + iy * ROWP;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            if (LAYOUT == ALINK_LAYOUT_NHWC_U8) raw[jj] = (float)((const uint8_t*)s.in)[base + goff[jj]];
            else                                raw[jj] = ((const float*)s.in)[base + goff[jj]];
        }
    };
    auto store_row = [&](int slot, const float (&raw)[2]) __attribute__((always_inline)) {
        char* const rb = smem + IOFF + slot * IMROWB;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const T v = (T)((raw[jj] - ssub[jj]) * s.mul);
            char* const dst = rb + soff[jj];
            *(T*)(soff[jj] >= 0 && soff[jj] < W * IMPX ? dst : sink) = v;
            *(T*)(soff[jj] >= 0 ? dst - IMPX + 6 : sink) = v;
            *(T*)(soff[jj] >= 2 * IMPX ? dst - 2 * IMPX + 12 : sink) = v;
        }
    };

    float raw[2];
    load_row(G0 - 3, raw);
#pragma unroll 1
    for (int k = 0; k < NP; ++k) {
        lds_done_then_barrier();
        store_row(k & (IR - 1), raw);                  // pixel row G0 - 3 + k
        load_row(G0 - 2 + k, raw);

        if (k >= 3 && k <= NP - 3) {
            // stem row g = G0 - 5 + k (>= -2) from the pixel rows parked in the three passes before
            const int r = (G0 - 5 + k + H) % H;
            const char* const rbm = smem + (r == 0 ? ZOFF : IOFF + ((k - 3) & (IR - 1)) * IMROWB);
            const char* const rbz = smem + IOFF + ((k - 2) & (IR - 1)) * IMROWB;
            const char* const rbp = smem + (r == H - 1 ? ZOFF : IOFF + ((k - 1) & (IR - 1)) * IMROWB);
            const char* const wa = (q < 2 ? rbm : rbz) + rec_off;
            const char* const wb = rbp + rec_off;
            char* const ob = smem + SOFF + (k % SR) * SPITCH + sw_off;
            const f32x4 sal0 = *(const f32x4*)(salpha + 16 * q + 8 * sch), sal1 = *(const f32x4*)(salpha + 16 * q + 8 * sch + 4);
            auto group = [&](auto X0, auto NX) __attribute__((always_inline)) {
                constexpr int x0 = decltype(X0)::a, nx = decltype(NX)::a;
                vec8 pa[nx], pb[nx];
#pragma unroll
                for (int i = 0; i < nx; ++i) {
                    pa[i] = *(const vec8*)(wa + 16 * IMPX * (x0 + i));
                    pb[i] = *(const vec8*)(wb + 16 * IMPX * (x0 + i));
                }
                f32x4 a0[nx], a1[nx];
#pragma unroll
                for (int i = 0; i < nx; ++i) {
                    a0[i] = mfma16<T>(swf[0][0], pa[i], f32x4{sbi[0], sbi[1], sbi[2], sbi[3]});      // the bias is the start value
                    a1[i] = mfma16<T>(swf[1][0], pa[i], f32x4{sbi[4], sbi[5], sbi[6], sbi[7]});
                }
#pragma unroll
                for (int i = 0; i < nx; ++i) {
                    a0[i] = mfma16<T>(swf[0][1], pb[i], a0[i]);
                    a1[i] = mfma16<T>(swf[1][1], pb[i], a1[i]);
                }
#pragma unroll
                for (int i = 0; i < nx; ++i) {
                    vec8 o8;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        o8[j] = (T)prelu<AMAX>(a0[i][j], sal0[j]);
                        o8[4 + j] = (T)prelu<AMAX>(a1[i][j], sal1[j]);
                    }
                    *(vec8*)(ob + 2048 * (x0 + i)) = o8;
                }
            };
            if (SHALF == 0) group(IC<0>{}, IC<4>{});
            else            group(IC<4>{}, IC<3>{});
        }

        if ((k & 1) && k >= 9) {
            // output row Y = R0 + (k - 9) / 2 from the t rows of the three passes before and the stem row of four passes before
            const int Y = R0 + ((k - 9) >> 1);
            const int y = Y % HO;
            int sb[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) sb[ky] = TOFF + ((k - 3 + ky) & (TR - 1)) * TPITCH;
            if (y == 0) sb[0] = ZOFF;
            const int scb = SOFF + ((k - 4) % SR) * SPITCH;
            f32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            auto frag = [&](int st, int t) __attribute__((always_inline)) -> vec8 {
                const int tap = st >> 1, ks = st & 1, ky = tap / 3, kx = tap % 3;
                return *(const vec8*)(smem + sb[ky] + loff2[kx == 2 ? 1 : 0][ks] + (kx == 1 ? ODDB : 0) + 2048 * t);
            };
            vec8 pf[2][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) pf[0][t] = frag(0, t);
            vec8 xs[2][4];
#pragma unroll
            for (int st = 0; st < 18; ++st) {
                if (st + 1 < 18) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) pf[(st + 1) & 1][t] = frag(st + 1, t);
                } else {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                        for (int t = 0; t < 4; ++t) xs[ks][t] = *(const vec8*)(smem + scb + scoff[ks] + 4096 * t);
                }
                const int tap = st >> 1, ks = st & 1;
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = mfma16<T>(w2r[tap][ks], pf[st & 1][t], acc[t]);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = mfma16<T>(ws[ks], xs[ks][t], acc[t]);

            // epilogue: bias, rounding; the lanes of the empty half tile store nothing (an ordinary predicated store)
            const f32x4 b4 = *(const f32x4*)(eb2 + cch * 32 + 8 * q + 4 * cct);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int x = 16 * t + d;
                const bool live = x < WO;
                const size_t el = ((size_t)Y * WO + (live ? x : 0)) * 64 + cch * 32 + 8 * q + 4 * cct;
                vec8 o8;
#pragma unroll
                for (int j = 0; j < 4; ++j) { o8[j] = (T)(acc[t][j] + b4[j]); o8[4 + j] = (T)0.f; }
                const i32x4 o4 = __builtin_bit_cast(i32x4, o8);
                if (live) *(i32x2*)((T*)p.out + el) = i32x2{o4[0], o4[1]};
            }
        }
    }
}

template <typename T, int LAYOUT, bool AMAX>
__global__ __launch_bounds__(NT, 1) void unit1_c64_kernel(const Unit1Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    // ---- once per workgroup: the zero pixels of the slots, the zero row, the pixel-record ring (the window elements beyond the
    // left / right border and the pads are never written again), the tables.  All of it is read after the first pass's barrier.
    for (int i = tid; i < TR * 8; i += NT) *(uint4*)(smem + TOFF + (i >> 3) * TPITCH + (i & 7) * 16) = uint4{0u, 0u, 0u, 0u};
    for (int i = tid; i < SR * 16; i += NT) {
        const int slot = i >> 4, side = (i >> 3) & 1, piece = i & 7;
        *(uint4*)(smem + SOFF + slot * SPITCH + (side ? (W + 1) * 128 : 0) + piece * 16) = uint4{0u, 0u, 0u, 0u};
    }
    for (int i = tid; i < (SPITCH + IR * IMROWB) / 16; i += NT) *(uint4*)(smem + ZOFF + i * 16) = uint4{0u, 0u, 0u, 0u};
    {
        float* const tbl = (float*)(smem + BOFF);
        for (int i = tid; i < 12 * 64; i += NT)
            tbl[i] = i < 9 * 64 ? p.b1[i] : (i < 10 * 64 ? p.a1[i - 9 * 64] : (i < 11 * 64 ? p.s.alpha[i - 10 * 64] : p.b2[i - 11 * 64]));
    }
    const long long nrows = (long long)p.N * HO;
    const int R0 = (int)(nrows * blockIdx.x / gridDim.x), R1 = (int)(nrows * (blockIdx.x + 1) / gridDim.x);
    const int NP = 2 * (R1 - R0) + 8;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // waves w and w + 4 share a SIMD: a 4-tile conv1 wave with a 3-tile stem wave, and the reverse
    if (wave < 4) {
        if ((wave >> 1) == 0) conv1_wave<T, AMAX, 0>(p, smem, wave & 1, 2 * R0, NP);
        else                  conv1_wave<T, AMAX, 1>(p, smem, wave & 1, 2 * R0, NP);
    } else {
        if (((wave - 4) >> 1) == 0) stem_conv2_wave<T, LAYOUT, AMAX, 1>(p, smem, wave - 4, R0, NP);
        else                        stem_conv2_wave<T, LAYOUT, AMAX, 0>(p, smem, wave - 4, R0, NP);
    }
}

// 0 = off, 1 = from FUSE_UNIT1_MIN_N images per launch, 2 = at every batch size
int g_fuse_unit1 = 1;

template <typename T, int LAYOUT>
hipError_t unit1_attr() {
    hipError_t e = hipFuncSetAttribute((const void*)unit1_c64_kernel<T, LAYOUT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)unit1_c64_kernel<T, LAYOUT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
}

template <typename T, int LAYOUT>
void unit1_launch_l(const Unit1Params& p, bool amax, unsigned grid, hipStream_t st) {
    if (amax) hipLaunchKernelGGL((unit1_c64_kernel<T, LAYOUT, true>), dim3(grid), dim3(NT), LDS_BYTES, st, p);
    else      hipLaunchKernelGGL((unit1_c64_kernel<T, LAYOUT, false>), dim3(grid), dim3(NT), LDS_BYTES, st, p);
}
template <typename T>
hipError_t unit1_launch(const Unit1Params& p, bool amax, unsigned grid, hipStream_t st) {
    switch (p.s.layout) {
        case ALINK_LAYOUT_NHWC_F32: unit1_launch_l<T, ALINK_LAYOUT_NHWC_F32>(p, amax, grid, st); break;
        case ALINK_LAYOUT_NCHW_F32: unit1_launch_l<T, ALINK_LAYOUT_NCHW_F32>(p, amax, grid, st); break;
        case ALINK_LAYOUT_NHWC_U8:  unit1_launch_l<T, ALINK_LAYOUT_NHWC_U8>(p, amax, grid, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

extern "C" void alink_debug_set_fuse_unit1(int mode) { g_fuse_unit1 = mode; }
int unit1_c64_mode() { return g_fuse_unit1; }

hipError_t unit1_c64_set_attributes() {
    hipError_t e;
    if ((e = unit1_attr<__bf16, ALINK_LAYOUT_NHWC_F32>()) != hipSuccess || (e = unit1_attr<__bf16, ALINK_LAYOUT_NCHW_F32>()) != hipSuccess ||
        (e = unit1_attr<__bf16, ALINK_LAYOUT_NHWC_U8>()) != hipSuccess)
        return e;
    if ((e = unit1_attr<_Float16, ALINK_LAYOUT_NHWC_F32>()) != hipSuccess || (e = unit1_attr<_Float16, ALINK_LAYOUT_NCHW_F32>()) != hipSuccess ||
        (e = unit1_attr<_Float16, ALINK_LAYOUT_NHWC_U8>()) != hipSuccess)
        return e;
    return hipSuccess;
}

// c1 / s: conv1 and the stem as launch_front_c64 would get them; c2: the unit's conv2 as launch_conv3x3_s2c64 would get it
// in its shortcut form (c2.in, c2.in2 and c1.out are not touched: t and the shortcut's operand stay in LDS)
bool unit1_c64_applies(int dtype, const ConvParams& c1, const StemParams& s, const ConvParams& c2) {
    if (dtype != ALINK_DT_BF16 && dtype != ALINK_DT_F16) return false;
    if (c1.ksz != 3 || c1.stride != 1 || c1.pad != 1 || c1.Cin != 64 || c1.Cout != 64 || c1.H != H || c1.W != W) return false;
    if (s.H != H || s.W != W || s.C0 != 64 || s.N != c1.N || c1.N <= 0 || c2.N != c1.N) return false;
    if (c1.splitk != 1 || c1.dact || c1.post_relu || c1.in2 || c1.resid || !c1.alpha || !c1.border_cls || c1.ablate || c1.stamps) return false;
    if (c2.ksz != 3 || c2.stride != 2 || c2.pad != 1 || c2.Cin != 64 || c2.Cout != 64 || c2.H != H || c2.W != W) return false;
    if (c2.splitk != 1 || c2.dact || c2.post_relu || c2.border_cls || !c2.in2 || c2.Cin2 != 64 || c2.alpha || c2.resid || c2.ablate || c2.stamps) return false;
    return (long long)c1.N * H * W * 64 < (1ll << 31);
}

hipError_t launch_unit1_c64(int dtype, const ConvParams& c1, const StemParams& s, const ConvParams& c2, bool slopes_le_1, hipStream_t st) {
    if (!unit1_c64_applies(dtype, c1, s, c2)) return hipErrorInvalidValue;
    Unit1Params p{};
    p.w1 = c1.wgt; p.b1 = c1.bias; p.a1 = c1.alpha; p.w2 = c2.wgt; p.b2 = c2.bias; p.out = c2.out; p.s = s; p.N = c1.N;
    const long long nrows = (long long)p.N * HO;
    const unsigned grid = (unsigned)(nrows < 256 ? nrows : 256);        // one persistent workgroup per CU
    if (dtype == ALINK_DT_BF16) return unit1_launch<__bf16>(p, slopes_le_1, grid, st);
    return unit1_launch<_Float16>(p, slopes_le_1, grid, st);
}

}  // namespace alink
