// augment.hip — the affine resampling of helpers.augment_data (reference code/helpers.py:114-141) on device.
//
// The reference calls tf.contrib.keras.preprocessing.image.random_rotation / random_shear / random_shift per image; each
// ends in scipy.ndimage.affine_transform(channel, A, offset, order=1, mode='nearest') once per channel.  Here one launch
// warps any number of output images: output i reads image src[i] of a table, maps its pixel (r, c) through the 2 x 3
// float64 matrix mat[i] and interpolates.  The arithmetic is scipy's (ni_interpolation.c / ni_splines.c), in float64
// with contraction off, so the float32 results are scipy's bit for bit:
//   y = (r m00 + c m01) + m02,  x = (r m10 + c m11) + m12;  each coordinate clamped to [0, n - 1] (mode 'nearest');
//   order 1: w0 = 1 - (y - floor y), w1 = 1 - w0 per axis; t = 0 + sum over the 2 x 2 taps (row-major) of (v * wy) * wx;
//   order 0: the tap floor(y + 0.5), floor(x + 0.5); t = 0 + v;
//   out = (float) t.
// A float32 coordinate path would miss by up to ~2e-3 on 0..255 pixels.  The coordinate and the weights are computed
// once per pixel and reused for all C channels: scipy computes the same numbers once per channel.
//
// One thread per output pixel (all channels), consecutive lanes along a row: the stores of a wave are contiguous.
// Nothing is reused across threads beyond what the caches catch, so there is no LDS.
#include "alink_common.h"

namespace alink {
namespace {

struct WarpP {
    const float* in;             // [n_in][H][W][C]
    const int* src;              // [n_out] source image of every output, or nullptr (output i reads image i)
    const double* mat;           // [n_out][2][3]
    const unsigned char* copy;   // [n_out] nonzero: a byte copy of the source, mat[i] unread; or nullptr
    float* out;                  // [n_out][H][W][C]
    int n_in, H, W, C, order;
    int blocks_per_image;
};

__global__ __launch_bounds__(256) void affine_warp_kernel(const WarpP p) {
#pragma clang fp contract(off)
    const int i = blockIdx.x / p.blocks_per_image;
    const int hw = p.H * p.W;
    const int pix = (blockIdx.x - i * p.blocks_per_image) * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int C = p.C;
    float* o = p.out + ((size_t)i * hw + pix) * C;
    const int s = p.src ? p.src[i] : i;
    if (s < 0 || s >= p.n_in) {                          // documented: a row of NaN, never a read out of the table
        for (int ch = 0; ch < C; ++ch) o[ch] = __builtin_nanf("");
        return;
    }
    const float* img = p.in + (size_t)s * hw * C;
    if (p.copy && p.copy[i]) {
        const float* a = img + (size_t)pix * C;
        for (int ch = 0; ch < C; ++ch) o[ch] = a[ch];
        return;
    }
    const int r = pix / p.W, c = pix - r * p.W;
    const double* m = p.mat + (size_t)i * 6;
    double y = ((double)r * m[0] + (double)c * m[1]) + m[2];
    double x = ((double)r * m[3] + (double)c * m[4]) + m[5];
    // scipy's map_coordinate for 'nearest': below 0 -> 0, above n - 1 -> n - 1 (a NaN coordinate goes to 0 here, so that
    // no index can leave the image)
    const double ymax = (double)(p.H - 1), xmax = (double)(p.W - 1);
    if (!(y >= 0.0)) y = 0.0;
    if (y > ymax) y = ymax;
    if (!(x >= 0.0)) x = 0.0;
    if (x > xmax) x = xmax;
    if (p.order == 0) {
        const int yi = (int)floor(y + 0.5), xi = (int)floor(x + 0.5);
        const float* a = img + ((size_t)yi * p.W + xi) * C;
        for (int ch = 0; ch < C; ++ch) o[ch] = (float)(0.0 + (double)a[ch]);
        return;
    }
    const double y0 = floor(y), x0 = floor(x);
    const double wy0 = 1.0 - (y - y0), wx0 = 1.0 - (x - x0);
    const double wy1 = 1.0 - wy0, wx1 = 1.0 - wx0;
    const int yi = (int)y0, xi = (int)x0;
    // the second tap leaves the image only where its weight is 0 (the coordinate sits on the last row / column): scipy
    // reads the edge pixel there ('nearest'), and so does this
    const int yj = yi + 1 < p.H ? yi + 1 : yi, xj = xi + 1 < p.W ? xi + 1 : xi;
    const float* a00 = img + ((size_t)yi * p.W + xi) * C;
    const float* a01 = img + ((size_t)yi * p.W + xj) * C;
    const float* a10 = img + ((size_t)yj * p.W + xi) * C;
    const float* a11 = img + ((size_t)yj * p.W + xj) * C;
    for (int ch = 0; ch < C; ++ch) {
        double t = 0.0;
        t += (double)a00[ch] * wy0 * wx0;
        t += (double)a01[ch] * wy0 * wx1;
        t += (double)a10[ch] * wy1 * wx0;
        t += (double)a11[ch] * wy1 * wx1;
        o[ch] = (float)t;
    }
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

int alink_affine_warp(const float* dev_in, int n_in, const int32_t* dev_src, const double* dev_mat, const uint8_t* dev_copy,
                      int n_out, int H, int W, int C, int order, float* dev_out, void* stream) {
    ALINK_REQUIRE(n_out >= 0 && n_in >= 0 && H > 0 && W > 0 && C > 0, ALINK_EINVAL, "bad argument");
    ALINK_REQUIRE(order == 0 || order == 1, ALINK_EINVAL, "order must be 0 or 1, got %d", order);
    if (n_out == 0) return ALINK_OK;
    ALINK_REQUIRE(dev_in && dev_mat && dev_out && n_in > 0, ALINK_EINVAL, "bad argument");
    ALINK_REQUIRE(dev_src || n_in >= n_out, ALINK_EINVAL, "without dev_src output i reads image i: n_in %d < n_out %d", n_in, n_out);
    ALINK_REQUIRE((void*)dev_in != (void*)dev_out, ALINK_EINVAL, "alink_affine_warp cannot run in place");
    const long long hw = (long long)H * W;
    ALINK_REQUIRE(hw * C < (1ll << 31), ALINK_EINVAL, "image too large");
    const long long bpi = (hw + 255) / 256;
    ALINK_REQUIRE(bpi * n_out < (1ll << 31), ALINK_EINVAL, "too many output images for one launch");
    DeviceGuard dg(device_of_pointer(dev_out));
    WarpP p{dev_in, dev_src, dev_mat, dev_copy, dev_out, n_in, H, W, C, order, (int)bpi};
    hipLaunchKernelGGL(affine_warp_kernel, dim3((unsigned)(bpi * n_out)), dim3(256), 0, (hipStream_t)stream, p);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
