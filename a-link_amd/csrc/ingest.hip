// ingest.hip — the raw-photo front end (reference code/face_preprocess.py:46-111, code/readDFW.py:28-62,82): one launch turns a
// RAGGED batch of photos, each of its own size, into network-sized float32 faces.
//
// The photos lie end to end in one packed table of HWC pixels (uint8 or float32); a descriptor per photo says where it starts,
// how large it is and what to do with it:
//   mode 0  crop + resize: the sub-image box = [x0, x1) x [y0, y1) resized to Ho x Wo by alink_resize_bilinear's own rule —
//           src_coord and bilinear_taps of resize_taps.h, computed relative to the box, so the float32 results are that
//           kernel's on the cropped array bit for bit.  src_coord clamps its taps to [0, size - 1]: none leaves the box.
//   mode 1  affine warp with a black border: m maps an OUTPUT pixel to source coordinates,
//               sx = (ox m0 + oy m1) + m2,  sy = (ox m3 + oy m4) + m5
//           in float64 with contraction off; per axis w0 = 1 - (s - floor s), w1 = 1 - w0; t = 0 + sum over the 2 x 2 taps
//           (row-major) of (v * wy) * wx, a tap outside the image contributing the value 0; the output is exactly 0 when
//           sx <= -1, sx >= W, sy <= -1 or sy >= H; out = (float) t.  That is scipy.ndimage.affine_transform(channel,
//           [[m4, m3], [m1, m0]], offset=[m5, m2], order=1, mode='grid-constant', cval=0) bit for bit (augment.hip is the
//           same arithmetic under mode='nearest').  A float32 coordinate path would miss by ~2e-3 on 0..255 pixels.
// The coordinate and the weights are computed once per pixel and reused for all C channels.
//
// One thread per output pixel (all channels), consecutive lanes along an output row: a wave's stores are contiguous, and the
// descriptor is uniform over a workgroup (ceil(Ho Wo / 256) workgroups per photo).  Nothing is reused across threads beyond
// what the caches catch, so there is no LDS.
// The kernel never reads outside the table: a descriptor that does not fit it (or, in mode 0, whose box is empty or leaves
// the image, or whose mode is unknown) yields a row of NaN, alink_affine_warp's convention.
#include "alink_common.h"
#include "resize_taps.h"

namespace alink {
namespace {

struct IngestP {
    const void* pix;                 // the packed table, total elements of T
    const AlinkIngestDesc* desc;     // [n]
    float* out;                      // [n][Ho][Wo][C] or [n][C][Ho][Wo]
    long long total;
    int C, Ho, Wo, nchw;
    int blocks_per_image;
};

template <typename T>
__global__ __launch_bounds__(256) void ingest_kernel(const IngestP p) {
#pragma clang fp contract(off)
    const int i = blockIdx.x / p.blocks_per_image;
    const int how = p.Ho * p.Wo;
    const int pix = (blockIdx.x - i * p.blocks_per_image) * 256 + threadIdx.x;
    if (pix >= how) return;
    const int C = p.C;
    // element ch of this pixel: o[ch * cs]
    float* o = p.nchw ? p.out + (size_t)i * C * how + pix : p.out + ((size_t)i * how + pix) * C;
    const size_t cs = p.nchw ? (size_t)how : 1;
    const AlinkIngestDesc& d = p.desc[i];
    const long long off = d.offset;
    const int H = d.H, W = d.W, mode = d.mode;
    // off + H W C <= total without a product that can overflow: H W < 2^62, and the right side is exact integer division
    bool ok = off >= 0 && off <= p.total && H >= 1 && W >= 1 && (mode == 0 || mode == 1) &&
              (unsigned long long)H * (unsigned long long)W <= (unsigned long long)(p.total - off) / (unsigned long long)C;
    const int bx0 = d.box[0], by0 = d.box[1], bx1 = d.box[2], by1 = d.box[3];
    if (mode == 0) ok = ok && bx0 >= 0 && by0 >= 0 && bx1 <= W && by1 <= H && bx0 < bx1 && by0 < by1;
    if (!ok) {
        for (int ch = 0; ch < C; ++ch) o[ch * cs] = __builtin_nanf("");
        return;
    }
    const T* img = (const T*)p.pix + off;
    const int oy = pix / p.Wo, ox = pix - oy * p.Wo;
    if (mode == 0) {
        int x0, x1, y0, y1;
        float fx, fy;
        src_coord(ox, bx1 - bx0, p.Wo, x0, x1, fx);
        src_coord(oy, by1 - by0, p.Ho, y0, y1, fy);
        const T* a00 = img + ((size_t)(by0 + y0) * W + (bx0 + x0)) * C;
        const T* a01 = img + ((size_t)(by0 + y0) * W + (bx0 + x1)) * C;
        const T* a10 = img + ((size_t)(by0 + y1) * W + (bx0 + x0)) * C;
        const T* a11 = img + ((size_t)(by0 + y1) * W + (bx0 + x1)) * C;
        for (int ch = 0; ch < C; ++ch)
            o[ch * cs] = bilinear_taps((float)a00[ch], (float)a01[ch], (float)a10[ch], (float)a11[ch], fx, fy);
        return;
    }
    const double sx = ((double)ox * d.m[0] + (double)oy * d.m[1]) + d.m[2];
    const double sy = ((double)ox * d.m[3] + (double)oy * d.m[4]) + d.m[5];
    // scipy's 'grid-constant': a coordinate in (-1, n) still blends with the border; beyond it (a NaN too) the pixel is cval
    if (!(sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H)) {
        for (int ch = 0; ch < C; ++ch) o[ch * cs] = 0.f;
        return;
    }
    const double yf = floor(sy), xf = floor(sx);
    const double wy0 = 1.0 - (sy - yf), wx0 = 1.0 - (sx - xf);
    const double wy1 = 1.0 - wy0, wx1 = 1.0 - wx0;
    const int yi = (int)yf, xi = (int)xf;                 // in [-1, n - 1]
    const bool iy0 = yi >= 0, iy1 = yi + 1 < H, ix0 = xi >= 0, ix1 = xi + 1 < W;
    // a tap outside the image is never addressed: its pointer stays on the image's first pixel and its value is 0
    const T* a00 = img + (iy0 && ix0 ? ((size_t)yi * W + xi) * C : 0);
    const T* a01 = img + (iy0 && ix1 ? ((size_t)yi * W + (xi + 1)) * C : 0);
    const T* a10 = img + (iy1 && ix0 ? ((size_t)(yi + 1) * W + xi) * C : 0);
    const T* a11 = img + (iy1 && ix1 ? ((size_t)(yi + 1) * W + (xi + 1)) * C : 0);
    for (int ch = 0; ch < C; ++ch) {
        const double v00 = iy0 && ix0 ? (double)a00[ch] : 0.0, v01 = iy0 && ix1 ? (double)a01[ch] : 0.0;
        const double v10 = iy1 && ix0 ? (double)a10[ch] : 0.0, v11 = iy1 && ix1 ? (double)a11[ch] : 0.0;
        double t = 0.0;
        t += v00 * wy0 * wx0;
        t += v01 * wy0 * wx1;
        t += v10 * wy1 * wx0;
        t += v11 * wy1 * wx1;
        o[ch * cs] = (float)t;
    }
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

int alink_ingest_faces(const void* dev_pixels, int src_dtype, int64_t total_elems, const AlinkIngestDesc* dev_desc, int n, int C,
                       int Ho, int Wo, int layout, float* dev_out, void* stream) {
    ALINK_REQUIRE(n >= 0 && C > 0 && Ho > 0 && Wo > 0 && total_elems >= 0, ALINK_EINVAL, "bad argument");
    ALINK_REQUIRE(src_dtype == 0 || src_dtype == 1, ALINK_EINVAL, "src_dtype must be 0 (uint8) or 1 (float32), got %d", src_dtype);
    ALINK_REQUIRE(layout == 0 || layout == 1, ALINK_EINVAL, "layout must be 0 (NHWC) or 1 (NCHW), got %d", layout);
    if (n == 0) return ALINK_OK;
    ALINK_REQUIRE(dev_pixels && dev_desc && dev_out, ALINK_EINVAL, "bad argument");
    const long long how = (long long)Ho * Wo;
    ALINK_REQUIRE(how < (1ll << 31) && how * C < (1ll << 40), ALINK_EINVAL, "output image too large");
    const long long bpi = (how + 255) / 256;
    ALINK_REQUIRE(bpi * n < (1ll << 31), ALINK_EINVAL, "too many output images for one launch");
    // the table is read while the faces are written: they must not share a byte
    const uintptr_t t0 = (uintptr_t)dev_pixels, t1 = t0 + (uintptr_t)total_elems * (src_dtype == 0 ? 1u : 4u);
    const uintptr_t o0 = (uintptr_t)dev_out, o1 = o0 + (uintptr_t)n * (uintptr_t)(how * C) * sizeof(float);
    ALINK_REQUIRE(o1 <= t0 || t1 <= o0, ALINK_EINVAL, "alink_ingest_faces: dev_out overlaps the pixel table");
    DeviceGuard dg(device_of_pointer(dev_out));
    IngestP p{dev_pixels, dev_desc, dev_out, (long long)total_elems, C, Ho, Wo, layout, (int)bpi};
    if (src_dtype == 0)
        hipLaunchKernelGGL(ingest_kernel<unsigned char>, dim3((unsigned)(bpi * n)), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(ingest_kernel<float>, dim3((unsigned)(bpi * n)), dim3(256), 0, (hipStream_t)stream, p);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
