// resnet50_bwd.hip — the small kernels of the VGGFace2 ResNet-50's input-gradient pass (resnet50.hip,
// alink_resnet50_input_grad).  The convolutions of that pass are conv_igemm / conv3x3_direct with transposed
// (and, for 3x3, flipped) folded weights and the ReLU' epilogue (`dact`); what has no forward twin is here:
//   * r50_grad_scale_kernel     the call's power-of-two gradient scale from max|dfeat| (f16 range, see below)
//   * r50_avgpool_bwd_kernel    d(avg_pool) spread over the 7 x 7 map, times the last unit's ReLU mask
//   * r50_relu_mask_kernel      identity units: the previous unit's ReLU mask on d(unit input), in place
//   * r50_scatter_mask_kernel   stride-2 units: d(unit input) from the small map to the even positions of the
//                               large one (zero elsewhere), times the previous unit's ReLU mask
//   * r50_maxpool_bwd_kernel    3x3/2 max-pool backward in GATHER form (no atomics), times the stem's ReLU mask
//   * r50_stem_bwd_kernel       the transposed 7x7 stride-2 convolution 64 -> 3 by output-pixel parity, on the matrix cores
//
// Gradient scale.  The gradient tensors are stored in the mode's 16-bit type.  d(loss)/d(feature) out of a pair
// scorer can be ~1e-6 and the average pool divides it by 49: below f16's normal range.  Every pass is linear in
// dfeat, so the call multiplies dfeat by 2^e with max|dfeat| 2^e / 49 in [1, 2) — exact — and the stem kernel
// multiplies the float32 result by 2^-e.  The scale lives in the caller's workspace (no host round trip).
#include "conv_device.h"

namespace alink {
namespace {

// one workgroup; scale[0] = 2^e, scale[1] = 2^-e.  A zero or non-finite maximum leaves e = 0.
__global__ __launch_bounds__(1024) void r50_grad_scale_kernel(const float* __restrict__ dfeat, int count, float inv_hw,
                                                              float* __restrict__ scale) {
    __shared__ float red[16];
    float m = 0.f;
    for (int i = threadIdx.x; i < count; i += 1024) m = fmaxf(m, fabsf(dfeat[i]));      // fmaxf drops a NaN
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
        m *= inv_hw;
        int e = 0;
        if (m > 0.f && m <= 3.4e38f) e = -ilogbf(m);
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
        scale[0] = ldexpf(1.f, e);
        scale[1] = ldexpf(1.f, -e);
    }
}

// dz[n][pos][c] = y[n][pos][c] > 0 ? dfeat[n][c] * 2^e / HW : 0; one thread = 8 channels of one position
template <typename T>
__global__ void r50_avgpool_bwd_kernel(const float* __restrict__ dfeat, const T* __restrict__ y, T* __restrict__ dz,
                                       const float* __restrict__ scale, int N, int HW, int C, float inv_hw) {
    typedef typename Vec8<T>::type vec8;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int c8n = C >> 3;
    if (i >= N * HW * c8n) return;
    const int c8 = i % c8n, n = i / (c8n * HW);
    const float mul = scale[0] * inv_hw;
    const f32x4 g0 = *(const f32x4*)(dfeat + (size_t)n * C + c8 * 8), g1 = *(const f32x4*)(dfeat + (size_t)n * C + c8 * 8 + 4);
    const vec8 a = *(const vec8*)(y + (size_t)i * 8);
    vec8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (T)((float)a[j] > 0.f ? (j < 4 ? g0[j] : g1[j - 4]) * mul : 0.f);
    *(vec8*)(dz + (size_t)i * 8) = o;
}

// g[i] = y[i] > 0 ? g[i] : 0, in place; one thread = 8 elements
template <typename T>
__global__ void r50_relu_mask_kernel(T* __restrict__ g, const T* __restrict__ y, long long count8) {
    typedef typename Vec8<T>::type vec8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count8) return;
    const vec8 a = *(const vec8*)(y + i * 8);
    vec8 v = *(const vec8*)(g + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)a[j] > 0.f ? v[j] : (T)0.f;
    *(vec8*)(g + i * 8) = v;
}

// out [N][H][W][C] <- in [N][Ho][Wo][C]: out[2 oy][2 ox] = y > 0 ? in[oy][ox] : 0, zero elsewhere (the transposed 1x1 ran on
// the small map: a stride-2 1x1 reads only the even positions); y = the stored forward tensor at out's positions
template <typename T>
__global__ void r50_scatter_mask_kernel(const T* __restrict__ in, const T* __restrict__ y, T* __restrict__ out, int N, int H,
                                        int W, int Ho, int Wo, int C) {
    typedef typename Vec8<T>::type vec8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c8n = C >> 3;
    if (i >= (long long)N * H * W * c8n) return;
    const int c8 = (int)(i % c8n);
    long long t = i / c8n;
    const int x = (int)(t % W); t /= W;
    const int yy = (int)(t % H);
    const int n = (int)(t / H);
    vec8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    if (!(yy & 1) && !(x & 1) && (yy >> 1) < Ho && (x >> 1) < Wo) {
        const vec8 g = *(const vec8*)(in + (((size_t)n * Ho + (yy >> 1)) * Wo + (x >> 1)) * C + c8 * 8);
        const vec8 a = *(const vec8*)(y + (size_t)i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)a[j] > 0.f ? g[j] : (T)0.f;
    }
    *(vec8*)(out + (size_t)i * 8) = v;
}

// MaxPooling2D((3,3), strides 2, 'valid') backward, gather form.  One thread = 8 channels of one pixel (y, x) of the
// stem map: it visits the at most 2 x 2 windows that cover the pixel and takes a window's gradient where the pixel is that
// window's FIRST maximum in row-major order (torch's rule).  The window's maximum is the stored pooled value, so the pixel
// is a maximum where it equals it, and the first one where no EARLIER element of the window equals it too; those are read
// only when some channel of the pixel is a positive maximum.  The stem's ReLU mask (stored activation > 0) is applied on
// the way: d0 is d(loss)/d(pre-ReLU stem output).
template <typename T>
__global__ void r50_maxpool_bwd_kernel(const T* __restrict__ y0, const T* __restrict__ pooled, const T* __restrict__ g,
                                       T* __restrict__ d0, int N, int H, int W, int C, int Hp, int Wp) {
    typedef typename Vec8<T>::type vec8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c8n = C >> 3;
    if (i >= (long long)N * H * W * c8n) return;
    const int c8 = (int)(i % c8n);
    long long t = i / c8n;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H);
    const int n = (int)(t / H);
    const vec8 me = *(const vec8*)(y0 + (size_t)i * 8);
    float v[8], acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = (float)me[j]; acc[j] = 0.f; }
    const int oy_lo = y > 0 ? (y - 1) >> 1 : 0, oy_hi = min(y >> 1, Hp - 1);
    const int ox_lo = x > 0 ? (x - 1) >> 1 : 0, ox_hi = min(x >> 1, Wp - 1);
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const size_t po = (((size_t)n * Hp + oy) * Wp + ox) * C + c8 * 8;
            const vec8 mx = *(const vec8*)(pooled + po);
            float m[8];
            bool take[8], any = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                m[j] = (float)mx[j];
                take[j] = v[j] > 0.f && v[j] == m[j];
                any = any || take[j];
            }
            if (!any) continue;
            const int kme = (y - 2 * oy) * 3 + (x - 2 * ox);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k >= kme) break;
                const vec8 w = *(const vec8*)(y0 + (((size_t)n * H + 2 * oy + k / 3) * W + 2 * ox + k % 3) * C + c8 * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) take[j] = take[j] && (float)w[j] != m[j];
            }
            const vec8 gv = *(const vec8*)(g + po);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += take[j] ? (float)gv[j] : 0.f;
        }
    vec8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (T)acc[j];
    *(vec8*)(d0 + (size_t)i * 8) = o;
}

// ---- stem backward ------------------------------------------------------------------------------------------------
// dpix[n][iy][ix][c] = 2^-e sum_{ky,kx,co} d0[n][oy][ox][co] w[ky][kx][c][co],  2 oy = iy + pad_t - ky, 2 ox = ix + pad_l - kx.
// Only taps of the pixel's parity reach it: ky = ky0 + 2 b with ky0 = (iy + pad_t) & 1, so 4 or 3 of the 7 rows, likewise in
// x: the four parity classes use 16 / 12 / 12 / 9 of the 49 taps (0.24 GFLOP per 224 x 224 image instead of the 0.94 of a
// convolution over a zero-inserted map).  blockIdx.y = class, so the tap set is uniform over the workgroup.
// It runs on the matrix cores (measured at 128 images, bf16: 1.08 ms; the same parity form on the VALU, weights as scalar
// operands, four pixels per thread, took 4.90 ms: its 16-byte loads 128 bytes apart kept the L1's address path busy).
// Per parity class the sum is a GEMM with M = 3 colour channels (padded to one 16-row tile),
// N = the pixels of the class, K = taps x 64: v_mfma_f32_16x16x32 with A = a weight fragment (row c, 8 of the 32 channels of
// one tap and channel half: [49][2][64 lanes][8] T, built at finalize, rows 3 .. 15 zero) and B = d0 at the 16 pixels of a
// tile (lane = pixel lr, channel group q: one 16-byte load straight from global memory — neighbouring taps and tiles re-read
// the same lines from L1).  One wave owns one row of one class: its 112 pixels are 7 tiles, 7 accumulators; a weight
// fragment is loaded once per tap and channel half and feeds the 7 MFMAs, whose 7 loads are in flight together.
constexpr int SB_TILES = 7;       // 16-pixel tiles per class row: rows of up to 224 pixels

template <typename T>
__global__ __launch_bounds__(256) void r50_stem_bwd_kernel(const T* __restrict__ d0, const T* __restrict__ wfrag,
                                                                float* __restrict__ dpix, const float* __restrict__ scale, int N,
                                                                int H, int W, int Ho, int Wo, int pad_t, int pad_l, int flip) {
    typedef typename Vec8<T>::type vec8;
    const int cls = blockIdx.y, py = cls >> 1, px = cls & 1;
    const int ky0 = (py + pad_t) & 1, kx0 = (px + pad_l) & 1;
    const int dy0 = (py + pad_t - ky0) >> 1, dx0 = (px + pad_l - kx0) >> 1;
    const int nty = ky0 ? 3 : 4, ntx = kx0 ? 3 : 4;
    const int JY = (H + 1) >> 1;
    const int lane = threadIdx.x & 63, lr = lane & 15, q = lane >> 4;
    const long long rowid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (rowid >= (long long)N * JY) return;
    const int n = (int)(rowid / JY), jy = (int)(rowid % JY);
    const int iy = 2 * jy + py;
    if (iy >= H) return;
    f32x4 acc[SB_TILES];
#pragma unroll
    for (int t = 0; t < SB_TILES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    vec8 zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = (T)0.f;
    for (int b = 0; b < nty; ++b) {
        const int oy = jy + dy0 - b;
        if ((unsigned)oy >= (unsigned)Ho) continue;                                // wave-uniform
        const T* row = d0 + ((size_t)n * Ho + oy) * Wo * 64 + 8 * q;
        for (int a = 0; a < ntx; ++a) {
            const T* wf = wfrag + ((size_t)((ky0 + 2 * b) * 7 + kx0 + 2 * a) * 2 * 64 + lane) * 8;
            const int oxb = lr + dx0 - a;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const vec8 wv = *(const vec8*)(wf + h * 64 * 8);
                vec8 dv[SB_TILES];
#pragma unroll
                for (int t = 0; t < SB_TILES; ++t) {
                    const int ox = 16 * t + oxb;
                    const bool ok = (unsigned)ox < (unsigned)Wo;
                    dv[t] = *(const vec8*)(row + (size_t)(ok ? ox : 0) * 64 + h * 32);
                    if (!ok) dv[t] = zero;
                }
#pragma unroll
                for (int t = 0; t < SB_TILES; ++t) acc[t] = mfma16<T>(wv, dv[t], acc[t]);
            }
        }
    }
    if (q != 0) return;                 // rows 0 .. 2 of the result (the colour channels) sit in lanes 0 .. 15, one pixel each
    const float inv = scale[1];
#pragma unroll
    for (int t = 0; t < SB_TILES; ++t) {
        const int ix = 2 * (16 * t + lr) + px;
        if (ix >= W) continue;
        float* o = dpix + (((size_t)n * H + iy) * W + ix) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[flip ? 2 - c : c] = acc[t][c] * inv;
    }
}

}  // namespace

hipError_t launch_r50_grad_scale(const float* dfeat, int count, int HW, float* scale, hipStream_t st) {
    if (count <= 0 || HW <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(r50_grad_scale_kernel, dim3(1), dim3(1024), 0, st, dfeat, count, 1.f / (float)HW, scale);
    return hipGetLastError();
}

hipError_t launch_r50_avgpool_bwd(int dtype, const float* dfeat, const void* y, void* dz, const float* scale, int N, int HW, int C,
                                  hipStream_t st) {
    const long long tot = (long long)N * HW * (C / 8);
    if (tot <= 0 || tot >= (1ll << 31) || C % 8) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((tot + 255) / 256)), block(256);
    typedef __bf16 B; typedef _Float16 F;
    if (dtype == ALINK_DT_BF16) hipLaunchKernelGGL(r50_avgpool_bwd_kernel<B>, grid, block, 0, st, dfeat, (const B*)y, (B*)dz, scale, N, HW, C, 1.f / (float)HW);
    else if (dtype == ALINK_DT_F16) hipLaunchKernelGGL(r50_avgpool_bwd_kernel<F>, grid, block, 0, st, dfeat, (const F*)y, (F*)dz, scale, N, HW, C, 1.f / (float)HW);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_r50_relu_mask(int dtype, void* g, const void* y, long long count, hipStream_t st) {
    if (count <= 0 || count % 8 || count / 8 / 256 >= (1ll << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((count / 8 + 255) / 256)), block(256);
    typedef __bf16 B; typedef _Float16 F;
    if (dtype == ALINK_DT_BF16) hipLaunchKernelGGL(r50_relu_mask_kernel<B>, grid, block, 0, st, (B*)g, (const B*)y, count / 8);
    else if (dtype == ALINK_DT_F16) hipLaunchKernelGGL(r50_relu_mask_kernel<F>, grid, block, 0, st, (F*)g, (const F*)y, count / 8);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_r50_scatter_mask(int dtype, const void* in, const void* y, void* out, int N, int H, int W, int Ho, int Wo, int C,
                                   hipStream_t st) {
    const long long tot = (long long)N * H * W * (C / 8);
    if (tot <= 0 || (tot + 255) / 256 >= (1ll << 31) || C % 8 || Ho != (H + 1) / 2 || Wo != (W + 1) / 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((tot + 255) / 256)), block(256);
    typedef __bf16 B; typedef _Float16 F;
    if (dtype == ALINK_DT_BF16) hipLaunchKernelGGL(r50_scatter_mask_kernel<B>, grid, block, 0, st, (const B*)in, (const B*)y, (B*)out, N, H, W, Ho, Wo, C);
    else if (dtype == ALINK_DT_F16) hipLaunchKernelGGL(r50_scatter_mask_kernel<F>, grid, block, 0, st, (const F*)in, (const F*)y, (F*)out, N, H, W, Ho, Wo, C);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_r50_maxpool_bwd(int dtype, const void* y0, const void* pooled, const void* g, void* d0, int N, int H, int W, int C,
                                  int Hp, int Wp, hipStream_t st) {
    const long long tot = (long long)N * H * W * (C / 8);
    // the windows must lie inside the map: 2 (Hp - 1) + 2 <= H - 1
    if (tot <= 0 || (tot + 255) / 256 >= (1ll << 31) || C % 8 || 2 * Hp + 1 > H || 2 * Wp + 1 > W || Hp < 1 || Wp < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((tot + 255) / 256)), block(256);
    typedef __bf16 B; typedef _Float16 F;
    if (dtype == ALINK_DT_BF16) hipLaunchKernelGGL(r50_maxpool_bwd_kernel<B>, grid, block, 0, st, (const B*)y0, (const B*)pooled, (const B*)g, (B*)d0, N, H, W, C, Hp, Wp);
    else if (dtype == ALINK_DT_F16) hipLaunchKernelGGL(r50_maxpool_bwd_kernel<F>, grid, block, 0, st, (const F*)y0, (const F*)pooled, (const F*)g, (F*)d0, N, H, W, C, Hp, Wp);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

int r50_stem_bwd_max_width() { return 2 * 16 * SB_TILES; }

hipError_t launch_r50_stem_bwd(int dtype, const void* d0, const void* wfrag, float* dpix, const float* scale, int N, int H, int W,
                               int Ho, int Wo, int pad_t, int pad_l, int flip, hipStream_t st) {
    const long long rows = (long long)N * ((H + 1) / 2);
    if (rows <= 0 || (rows + 3) / 4 >= (1ll << 31) || pad_t < 0 || pad_l < 0 || pad_t > 6 || pad_l > 6 || Ho != (H + 1) / 2 ||
        Wo != (W + 1) / 2 || (W + 1) / 2 > 16 * SB_TILES)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + 3) / 4), 4), block(256);
    typedef __bf16 B; typedef _Float16 F;
    if (dtype == ALINK_DT_BF16) hipLaunchKernelGGL(r50_stem_bwd_kernel<B>, grid, block, 0, st, (const B*)d0, (const B*)wfrag, dpix, scale, N, H, W, Ho, Wo, pad_t, pad_l, flip);
    else if (dtype == ALINK_DT_F16) hipLaunchKernelGGL(r50_stem_bwd_kernel<F>, grid, block, 0, st, (const F*)d0, (const F*)wfrag, dpix, scale, N, H, W, Ho, Wo, pad_t, pad_l, flip);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace alink
