// resize_taps.h — the tap rule and the roundings of the bilinear resize (cv2.resize INTER_LINEAR, code/committee.py:22-26),
// shared by every kernel that must produce alink_resize_bilinear's bits: noise.hip (resize, its adjoint, perturb + resize)
// and ingest.hip (crop + resize of a ragged batch).
#pragma once
#include <hip/hip_runtime.h>

namespace alink {

// OpenCV's pixel-centre mapping: f = (d + 0.5) * (src / dst) - 0.5, s = floor(f), f -= s, clamped so
// that s in [0, src - 1] with weight 0 on the clamped side; horizontal pass then vertical pass.
__device__ __forceinline__ void src_coord(int d, int src, int dst, int& s0, int& s1, float& w) {
    float f = (float)(((double)d + 0.5) * ((double)src / (double)dst) - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
    w = f;
}

// The horizontal pass on both rows, then the vertical one:
//     r0 = a00 * (1 - fx) + a01 * fx,   r1 = a10 * (1 - fx) + a11 * fx,   out = r0 * (1 - fy) + r1 * fy
// with the roundings PINNED to the ones resize_kernel has always compiled to — each horizontal pass one fused multiply-add onto
// the rounded first product, the vertical pass two rounded products and an add — because which of two products the compiler
// contracts into an fma depends on the code around the expression: left to it, perturb_resize_kernel fused the vertical pass,
// resize_kernel did not, and the two disagreed in the last bit.
__device__ __forceinline__ float bilinear_taps(float a00, float a01, float a10, float a11, float fx, float fy) {
#pragma clang fp contract(off)
    const float r0 = __builtin_fmaf(a01, fx, a00 * (1.f - fx));
    const float r1 = __builtin_fmaf(a11, fx, a10 * (1.f - fx));
    return r0 * (1.f - fy) + r1 * fy;
}

}  // namespace alink
