// unit_c64.hip — one plain IR residual unit at 56 x 56 x 64 (stage 1, units 2 and 3) in ONE rolling-row launch:
//
//     t = PReLU(conv1(x) + b1[border class])          y = conv2(t) + b2 + x
//
// As two conv3x3_linear<T, 56, 2> launches a unit moves 585 MB per 292 images through HBM (conv1 reads x and writes t,
// conv2 reads t, re-reads x as its residual and writes y); only x in and y out (234 MB) have to cross it.  K is nine
// K-steps, so those launches also spend half of a workgroup's life in prologue and epilogue.  Here:
//
//   * one persistent 8-wave workgroup per CU owns a contiguous range of output rows of the batch seen as one tall image
//     (N * 56 rows) and rolls through image boundaries; a PASS is two rows = 112 pixels = seven whole 16-pixel MFMA tiles;
//   * waves 0..3 compute conv1, waves 4..7 conv2; each holds the folded weights of one 32-channel output group of its
//     convolution in registers (144 VGPRs: two waves per SIMD fit).  A channel group's seven tiles are split 4 + 3 between
//     two waves, and every SIMD hosts a 4-tile conv1 wave with a 3-tile conv2 wave or the reverse: 7 x 2 x 18 MFMAs each;
//   * x rows arrive by LDS-DMA one pass ahead into a ring of 8 row slots that also serves conv2's residual; conv1 writes
//     its t rows into a ring of 6 slots in the layout conv2's ds_read_b128 expects.  conv2 runs two passes behind conv1:
//     in pass k conv1 makes t rows R0 - 1 + 2k, R0 + 2k and conv2 makes output rows R0 + 2k - 4, R0 + 2k - 3 (R0: the
//     range's first row), so a range starting mid-image first computes the one t row above its first output row;
//   * ONE barrier per pass.  Image borders are done by address as in conv3x3_linear.hip: a lane whose tap crosses a row
//     end or an image's top / bottom adds border bits above bit 17 to its operand address, outside the LDS allocation,
//     where a DS read returns zero (the contract linear_check_contract probes; the dispatch requires the linear-tile
//     variant, which is only chosen where the probe passed).  Rows outside the batch are DMA'd from the zero page.
//
// Bit-identical to the two conv3x3_linear launches: the same packed weight rows and delta() lane permutation, the same
// (tap, K half) walk with the same 8-channel K slices on the same MFMA positions, conv1's epilogue (f32 accumulator + bias
// by border class, PReLU as v > 0 ? v : v * a, rounding to T) and conv2's (accumulator + bias + (float)residual, rounding).
#include "conv_device.h"

namespace alink {
namespace {

constexpr int W = 56;
constexpr int NT = 512;
constexpr int ROWB = W * 128;                 // a row slot: 56 pixels x 64 channels x 2 B, no padding
constexpr int XR = 8, TR = 6;                 // x / t ring slots
constexpr int TBL = 4096;                     // tables first (b1 by class, b2, PReLU slopes): no operand address below 0
constexpr int XOFF = TBL, TOFF = XOFF + XR * ROWB;
constexpr size_t LDS_BYTES = (size_t)TOFF + TR * ROWB;

struct UnitParams {
    const void*  x;       // [N][56][56][64] T: the unit's input and conv2's residual
    const void*  w1;      // [64][576] T, rows permuted (as for conv3x3_linear)
    const float* b1;      // [9][64] by border class
    const float* a1;      // [64] PReLU slopes
    const void*  w2;
    const float* b2;      // [64]
    void*        out;     // [N][56][56][64] T
    const void*  zero;    // >= 128 B of zeros
    int N;
};

// the slot-relative byte offset of pixel column c, 8-channel piece j: 16-B pieces XOR-swizzled by (c >> 1) & 7
__device__ __forceinline__ int slot_off(int c, int j) { return c * 128 + ((j ^ ((c >> 1) & 7)) << 4); }

// One wave's whole life.  CONV 1: conv1 (writes t rows into the ring, stages the x rows); CONV 2: conv2 (stores y).
// HALF 0: the pass's tiles 0..3 (row 0 and the tile that straddles the rows), HALF 1: tiles 4..6 (row 1).
template <typename T, int CONV, int HALF>
__device__ __forceinline__ void unit_wave(const UnitParams& p, char* smem, int ch, long long r0, int npairs) {
    typedef typename Vec8<T>::type vec8;
    constexpr int NTL = HALF == 0 ? 4 : 3;
    constexpr int U0 = HALF == 0 ? 0 : 4;            // first tile of the pass this wave computes
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = lane >> 4, lr = lane & 15;
    const int d = delta(lr);
    const long long nrows = (long long)p.N * W;

    const T* __restrict__ gw = (const T*)(CONV == 1 ? p.w1 : p.w2);
    vec8 wr[2][9][2];                                 // [channel tile][tap][K half], as conv3x3_c64
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                wr[ct][tap][ks] = *(const vec8*)(gw + (size_t)(ch * 32 + 16 * ct + lr) * 576 + tap * 64 + ks * 32 + 8 * q);

    // operand offsets: pixel P = 16 u + d of the pass (u = 0..6), row r = P >= 56, column c = P - 56 r; tap (ky, kx)
    // reads slot(row r + ky - 1) at column c + kx - 1.  With pos = d + kx - 1, rows 0 read  slot + 2048 u + lo, rows 1
    // read slot - 7168 + 2048 u + (lo ^ 64): 56 / 2 = 28 = 4 (mod 8) flips bit 2 of the swizzle term.
    int lo[3][2];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pos = d + kx - 1;
            const int v = pos * 128 + ((((ks << 2) | q) ^ ((pos >> 1) & 7)) << 4);
            lo[kx][ks] = HALF == 0 ? v : (v ^ 64);
        }
    const bool sel3 = HALF == 0 && d >= 8;             // tile 3: the lane's pixel lies in row 1
    const int x64 = sel3 ? 64 : 0;
    // border code per local tile: bit 0 row 0, bit 1 row 1, bit 2 column 0, bit 3 column 55
    unsigned bcode = 0;
#pragma unroll
    for (int u = 0; u < NTL; ++u) {
        const int P = 16 * (U0 + u) + d, r = P >= W ? 1 : 0, c = P - W * r;
        bcode |= ((r ? 2u : 1u) | (c == 0 ? 4u : 0u) | (c == W - 1 ? 8u : 0u)) << (4 * u);
    }

    const int bslot = CONV == 1 ? XOFF : TOFF;
    constexpr int RING = CONV == 1 ? XR : TR;
    const float* const eb1 = (const float*)smem;
    const float* const eb2 = eb1 + 9 * 64;
    const float* const ea1 = eb2 + 64;
    const T* __restrict__ gx = (const T*)p.x;
    const T* __restrict__ gz = (const T*)p.zero;

    // x rows [R0 - 2 + 2 j, +1] (the rows pass j - 1 adds to the window) -> slots (2 j, 2 j + 1) mod 8; 14 wave units of
    // 8 pixels dealt to the four conv1 waves
    auto stage_pair = [&](int j) {
        const int w4 = ch + 2 * HALF;                  // 0..3 among the conv1 waves
        for (int uidx = w4; uidx < 14; uidx += 4) {
            const int ri = uidx / 7, seg = uidx - ri * 7;
            const long long row = r0 - 2 + 2 * j + ri;
            const int slot = (2 * j + ri) % XR;
            const int px = seg * 8 + (lane >> 3);
            const int piece = (lane & 7) ^ ((px >> 1) & 7);
            const bool ok = row >= 0 && row < nrows;
            const T* src = ok ? gx + ((size_t)(row * W + px) * 64 + piece * 8) : gz + (lane & 7) * 8;
            dma16(src, smem + XOFF + slot * ROWB + seg * 1024);
        }
    };
    if (CONV == 1) stage_pair(0), stage_pair(1);       // pass 0 reads x rows R0 - 2 .. R0 + 1

    const int NP = npairs + 2;
#pragma unroll 1
    for (int k = 0; k < NP; ++k) {
        // conv1 waves wait for everything: what they have in flight are the DMAs of the rows this pass reads; the conv2
        // waves leave the stores of the pass before in flight, which nobody in the kernel reads
        if (CONV == 1) wait_then_barrier<0>();
        else           wait_then_barrier<NTL>();
        // this pass: conv1 rows ya = R0 - 1 + 2k (+1), window slots (2k .. 2k + 3) of x; conv2 rows ya = R0 + 2k - 4 (+1),
        // window slots (2k - 4 .. 2k - 1) of t
        const bool active = CONV == 1 ? k <= npairs : k >= 2;
        if (CONV == 1 && k + 1 <= npairs) stage_pair(k + 2);
        if (!active) continue;
        const long long ya = CONV == 1 ? r0 - 1 + 2 * k : r0 + 2 * k - 4;
        const int s0 = CONV == 1 ? 2 * k : 2 * k - 4;  // ring position of window row 0
        int sb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) sb[i] = bslot + ((s0 + i) % RING) * ROWB;
        const int m0 = (int)((ya + W) % W), m1 = (int)((ya + 1) % W);     // rows in their images (ya >= -1)
        const unsigned topm = (m0 == 0 ? 1u : 0u) | (m1 == 0 ? 2u : 0u);
        const unsigned botm = (m0 == W - 1 ? 1u : 0u) | (m1 == W - 1 ? 2u : 0u);

        f32x4 acc[2][NTL];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int u = 0; u < NTL; ++u) acc[ct][u] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto fetch = [&](vec8 (&pf)[NTL], int st) {
            const int tap = st >> 1, ks = st & 1, ky = tap / 3, kx = tap % 3;
            const unsigned tb = (ky == 0 ? topm : (ky == 2 ? botm : 0u)) | (kx == 0 ? 4u : 0u) | (kx == 2 ? 8u : 0u);
            unsigned bnow = bcode;
            asm volatile("" : "+v"(bnow));
            const int blo = sb[ky], bhi = sb[ky + 1] - ROWB;
#pragma unroll
            for (int u = 0; u < NTL; ++u) {
                const unsigned t = bnow & (tb << (4 * u));
                const int far = (int)(t << (18 - 4 * u));
                int a;
                if (HALF == 1)      a = bhi + lo[kx][ks] + 2048 * (U0 + u);
                else if (u < 3)     a = blo + lo[kx][ks] + 2048 * u;
                else                a = (sel3 ? bhi : blo) + (lo[kx][ks] ^ x64) + 2048 * 3;
                pf[u] = *(const vec8*)(smem + (a + far));
            }
        };
        vec8 pf[2][NTL];
        fetch(pf[0], 0);
#pragma unroll
        for (int st = 0; st < 18; ++st) {
            if (st + 1 < 18) fetch(pf[(st + 1) & 1], st + 1);
            const int tap = st >> 1, ks = st & 1;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int u = 0; u < NTL; ++u) acc[ct][u] = mfma16<T>(wr[ct][tap][ks], pf[st & 1][u], acc[ct][u]);
        }

        // epilogue: pixel (row ya + r, column c), channels 32 ch + 8 q .. + 7 = one 16-B piece (4 ch + q)
        const int jp = 4 * ch + q;
        if (CONV == 1) {
            const int ts0 = TOFF + ((2 * k) % TR) * ROWB, ts1 = TOFF + ((2 * k + 1) % TR) * ROWB;
            const f32x4 a0 = *(const f32x4*)(ea1 + ch * 32 + 8 * q), a1 = *(const f32x4*)(ea1 + ch * 32 + 8 * q + 4);
#pragma unroll
            for (int u = 0; u < NTL; ++u) {
                const int P = 16 * (U0 + u) + d, r = P >= W ? 1 : 0, c = P - W * r;
                const int m = r ? m1 : m0;
                const int cls = (m == 0 ? 0 : (m == W - 1 ? 2 : 1)) * 3 + (c == 0 ? 0 : (c == W - 1 ? 2 : 1));
                const f32x4 b0 = *(const f32x4*)(eb1 + cls * 64 + ch * 32 + 8 * q);
                const f32x4 b1 = *(const f32x4*)(eb1 + cls * 64 + ch * 32 + 8 * q + 4);
                float v[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { v[j] = acc[0][u][j] + b0[j]; v[4 + j] = acc[1][u][j] + b1[j]; }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = v[j] > 0.f ? v[j] : v[j] * a0[j];
                    v[4 + j] = v[4 + j] > 0.f ? v[4 + j] : v[4 + j] * a1[j];
                }
                vec8 o8;
#pragma unroll
                for (int i = 0; i < 8; ++i) o8[i] = (T)v[i];
                *(vec8*)(smem + (r ? ts1 : ts0) + slot_off(c, jp)) = o8;
            }
        } else {
            // residual: x rows ya, ya + 1 sit at x ring positions 2k - 2, 2k - 1
            const int xs0 = XOFF + ((2 * k - 2) % XR) * ROWB, xs1 = XOFF + ((2 * k - 1) % XR) * ROWB;
            const f32x4 b0 = *(const f32x4*)(eb2 + ch * 32 + 8 * q), b1 = *(const f32x4*)(eb2 + ch * 32 + 8 * q + 4);
            vec8 res[NTL];
#pragma unroll
            for (int u = 0; u < NTL; ++u) {
                const int P = 16 * (U0 + u) + d, r = P >= W ? 1 : 0, c = P - W * r;
                res[u] = *(const vec8*)(smem + (r ? xs1 : xs0) + slot_off(c, jp));
            }
#pragma unroll
            for (int u = 0; u < NTL; ++u) {
                const int P = 16 * (U0 + u) + d, r = P >= W ? 1 : 0, c = P - W * r;
                float v[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { v[j] = acc[0][u][j] + b0[j]; v[4 + j] = acc[1][u][j] + b1[j]; }
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] += (float)res[u][i];
                vec8 o8;
#pragma unroll
                for (int i = 0; i < 8; ++i) o8[i] = (T)v[i];
                *(vec8*)((T*)p.out + (size_t)((ya + r) * W + c) * 64 + ch * 32 + 8 * q) = o8;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(NT, 1) void unit_c64_kernel(const UnitParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    {
        float* const eb1 = (float*)smem;
        for (int i = tid; i < 9 * 64 + 64 + 64; i += NT)
            eb1[i] = i < 9 * 64 ? p.b1[i] : (i < 10 * 64 ? p.b2[i - 9 * 64] : p.a1[i - 10 * 64]);
    }
    // the tables are read after the first pass's barrier
    const long long pairs = (long long)p.N * (W / 2);
    const int nwg = gridDim.x;
    const int lid = xcd_remap(blockIdx.x, nwg);        // neighbouring ranges (shared halo rows) on one XCD's L2
    const long long p0 = pairs * lid / nwg, p1 = pairs * (lid + 1) / nwg;
    const long long r0 = 2 * p0;
    const int npairs = (int)(p1 - p0);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, half = (wave >> 1) & 1;
    // waves w and w + 4 share a SIMD: a 4-tile conv1 wave with a 3-tile conv2 wave, and the reverse
    if (wave < 4) {
        if (half == 0) unit_wave<T, 1, 0>(p, smem, ch, r0, npairs);
        else           unit_wave<T, 1, 1>(p, smem, ch, r0, npairs);
    } else {
        if (half == 0) unit_wave<T, 2, 1>(p, smem, ch, r0, npairs);
        else           unit_wave<T, 2, 0>(p, smem, ch, r0, npairs);
    }
}

}  // namespace

hipError_t unit_c64_set_attributes() {
    hipError_t e = hipFuncSetAttribute((const void*)unit_c64_kernel<__bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)unit_c64_kernel<_Float16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    return e;
}

bool unit_c64_applies(int dtype, const ConvParams& c1, const ConvParams& c2) {
    if (dtype != ALINK_DT_BF16 && dtype != ALINK_DT_F16) return false;
    auto plain = [](const ConvParams& c) {
        return c.ksz == 3 && c.stride == 1 && c.pad == 1 && c.H == W && c.W == W && c.Cin == 64 && c.Cout == 64 &&
               c.splitk == 1 && !c.dact && !c.post_relu && !c.in2 && !c.ablate && !c.stamps && c.N > 0;
    };
    return plain(c1) && plain(c2) && c1.N == c2.N && c1.alpha && c1.border_cls && !c1.resid && !c2.alpha && !c2.border_cls &&
           c2.resid == c1.in && (long long)c1.N * W * W * 64 < (1ll << 31);
}

// c1: the unit's conv1 launch as it would be made (its `out` is not written), c2: its conv2 (in = c1.out, resid = c1.in)
hipError_t launch_unit_c64(int dtype, const ConvParams& c1, const ConvParams& c2, hipStream_t st) {
    if (!unit_c64_applies(dtype, c1, c2)) return hipErrorInvalidValue;
    UnitParams p{};
    p.x = c1.in; p.w1 = c1.wgt; p.b1 = c1.bias; p.a1 = c1.alpha;
    p.w2 = c2.wgt; p.b2 = c2.bias; p.out = c2.out; p.zero = c1.zero; p.N = c1.N;
    const long long pairs = (long long)p.N * (W / 2);
    const unsigned grid = (unsigned)(pairs < 256 ? pairs : 256);                 // one persistent workgroup per CU
    if (dtype == ALINK_DT_BF16) hipLaunchKernelGGL(unit_c64_kernel<__bf16>, dim3(grid), dim3(NT), LDS_BYTES, st, p);
    else                        hipLaunchKernelGGL(unit_c64_kernel<_Float16>, dim3(grid), dim3(NT), LDS_BYTES, st, p);
    return hipGetLastError();
}

}  // namespace alink
