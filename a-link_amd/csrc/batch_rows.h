// batch_rows.h — the pool rows and the one squared-distance summation order that batch.hip (ranked batch selection) and
// density.hip (information density, the ranked batch's cold start) share.
//
// One summation order.  Element e of a row belongs to lane (e / 4) % 64, which adds its elements in ascending order with one
// fused multiply-add each (acc = fma(x - p, x - p, acc)); the 64 lane sums meet in an xor butterfly (32, 16, ..., 1), which
// gives every lane the same bits.  Rows in LDS are padded with zeros to a multiple of four floats, and a row's elements at
// or past D load as 0, so a padding term is fma(0, 0, acc) = acc.  That order is a function of D alone: the same in every
// kernel of both files, for vector and scalar loads, and for rows formed on the fly as |left - right| (one rounded
// subtraction, the bits the materialised row would hold).
#pragma once
#include "alink_common.h"

namespace alink {
namespace {

constexpr int RB_MAX_D = 8192;             // the picked row (and a labelled tile) in 32 KB of LDS
constexpr int RB_WG_ROWS = 32;             // init kernel: pool rows per workgroup, eight per wave

// the pool: an (N, D) row table (li == nullptr), or row n = |x[li[n]] - r[ri[n]]| from a left and a right feature table
struct RbRows {
    const float* x;
    const float* r;
    const int32_t* li;
    const int32_t* ri;
    int D;
};
struct RbRow { const float* a; const float* b; };

template <bool PAIR>
__device__ __forceinline__ RbRow rb_row(const RbRows& t, long long n) {
    RbRow p;
    if constexpr (PAIR) {
        p.a = t.x + (size_t)t.li[n] * t.D;
        p.b = t.r + (size_t)t.ri[n] * t.D;
    } else {
        p.a = t.x + (size_t)n * t.D;
        p.b = nullptr;
    }
    return p;
}

template <bool PAIR>
__device__ __forceinline__ float rb_elem(const RbRow& p, int e) {
    if constexpr (PAIR) return fabsf(p.a[e] - p.b[e]);
    else return p.a[e];
}

// elements e0 .. e0 + 3 of a row (e0 a multiple of 4 below D); those at or past D come back as 0
template <bool PAIR, bool VEC>
__device__ __forceinline__ float4 rb_quad(const RbRow& p, int e0, int D) {
    if constexpr (VEC) {                    // D is a multiple of 4 and the tables are 16-byte aligned
        float4 v = *(const float4*)(p.a + e0);
        if constexpr (PAIR) {
            const float4 w = *(const float4*)(p.b + e0);
            v.x = fabsf(v.x - w.x); v.y = fabsf(v.y - w.y); v.z = fabsf(v.z - w.z); v.w = fabsf(v.w - w.w);
        }
        return v;
    } else {
        float4 v;
        v.x = rb_elem<PAIR>(p, e0);
        v.y = e0 + 1 < D ? rb_elem<PAIR>(p, e0 + 1) : 0.f;
        v.z = e0 + 2 < D ? rb_elem<PAIR>(p, e0 + 2) : 0.f;
        v.w = e0 + 3 < D ? rb_elem<PAIR>(p, e0 + 3) : 0.f;
        return v;
    }
}

__device__ __forceinline__ float rb_acc(float s, const float4& x, const float4& p) {
    float d;
    d = x.x - p.x; s = __builtin_fmaf(d, d, s);
    d = x.y - p.y; s = __builtin_fmaf(d, d, s);
    d = x.z - p.z; s = __builtin_fmaf(d, d, s);
    d = x.w - p.w; s = __builtin_fmaf(d, d, s);
    return s;
}

// the 64 lane sums in the xor butterfly (32, 16, ..., 1): every lane ends with the same bits
__device__ __forceinline__ float rb_wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// s[4 a + b] = this lane's share of the distance between pool row a and labelled row b of a 4 x 4 block.  The 64 lanes' shares
// of every distance meet in the butterfly of a plain wave sum (levels 32, 16, ..., 1: the same additions, so the same bits),
// but packed: at each of the first four levels a lane keeps half of the sums it holds and hands the other half to its partner,
// 15 + 2 exchanges instead of 16 x 6.  Lane L ends with the total of a = L >> 4, b = (L >> 2) & 3.
template <int HELD>                     // one level: HELD sums held, partner at lane distance 2 HELD (a template: every index a constant)
__device__ __forceinline__ void rb_fold(float (&s)[16], int lane) {
    const bool up = (lane & (2 * HELD)) != 0;
#pragma unroll
    for (int j = 0; j < HELD / 2; ++j) {
        const float keep = up ? s[j + HELD / 2] : s[j];
        const float send = up ? s[j] : s[j + HELD / 2];
        s[j] = keep + __shfl_xor(send, 2 * HELD, 64);
    }
}
__device__ __forceinline__ float rb_block_pair_sums(float (&s)[16], int lane) {
    rb_fold<16>(s, lane);
    rb_fold<8>(s, lane);
    rb_fold<4>(s, lane);
    rb_fold<2>(s, lane);
    float v = s[0];
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

}  // namespace
}  // namespace alink
