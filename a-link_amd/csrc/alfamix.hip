// alfamix.hip — ALFA-Mix (Parvaneh et al. 2022, "Active learning by feature mixing") through the pair head of head.hip: does the
// head's decision for a pair flip when its feature d = |l - r| is pulled a short way towards an anchor (the mean labelled row
// of a class)?  EXTENSION: the reference takes its strategies from modAL, which has no such sampler.
//
// The rule is pinned in include/alink_hip.h (alink_head_feature_mix).  In short, with z1, a1, z2, a2, z3, probs the forward's
// and yhat its argmax (ties to class 0; one output: p > 0.5):
//     u = (W3[:,0] - W3[:,1]) . [z2 > 0]  (one output: W3[:,0] . [z2 > 0]),   v = (u W2^T) . [z1 > 0],   q = v W1^T
//     g = q if yhat = 1 else -q  (one output: -q if yhat = 1 else q),   G = |g|_2
//     per anchor a:  z = anchor_a - d,  Z = |z|_2,  s = eps Z / G,  t = s g,
//                    delta_e = min(max(t_e, min(z_e, 0)), max(z_e, 0))   (0 when G == 0 or G, Z not finite),  mixed_a = d + delta
// and the forward's arithmetic again on every mixed row.
//
// head_mix_kernel<CT> is head_egl_kernel<CT> carried on (32 pairs per workgroup, v_mfma_f32_32x32x2_f32, the same packed weights,
// k order, layer-2 split, sum order and softmax expression: its probabilities are the forward's bit for bit).  v under the z1
// mask is staged in the packed A-operand layout as there; a fourth MFMA GEMM (M = 32 pairs, K = h1, N = D) forms q from the
// packed W1^T copy and keeps it in registers, wave w owning the 32-column tiles w T .. w T + T - 1, T = ceil(ceil(D / 32) / 4).
// Per anchor the row d is staged again by index into the layer-1 image (D <= 512: the whole row in one chunk), mixed in place
// by the lane that holds q at that element, and layers 1-3 run on the image as they did on d.
//
// Sum orders, fixed by (D, h1, h2, A) alone — no atomics, a pair's outputs do not depend on P, on its tile or on its place in it:
//     q[e]    one MFMA chain over k = 0 .. h1 - 1 ascending, two k per instruction (the k order of layers 1 and 2)
//     G^2, Z^2  tile_row_sumsq's order over the D elements: share j of 8 adds the 8-element blocks j, j + 8, ... ascending, a
//             block in ascending e, one fused multiply-add per element; the shares meet in an xor butterfly (1, 2, 4).
//             z_e = fl(anchor_e - d_e) is rounded before it is squared, and is the z_e of the clamp.
//     G = fl(sqrt(G^2)), Z = fl(sqrt(Z^2)), s = fl(fl(eps Z) / G), t_e = fl(s g_e), mixed_e = fl(d_e + delta_e)
#include "head_handle.h"

using namespace alink;

namespace {

struct HeadMix {
    const float *L, *R;
    const int32_t *li, *ri;
    long long P;
    const float *w1p, *b1, *w2p, *w2tp, *w1tp, *b2, *w3, *b3;
    const float* anchors;         // [A][D]
    int A;
    float eps;
    float* probs;                 // [P][od]; each of the four may be nullptr
    uint8_t* flip;                // [P]
    float* mixed_probs;           // [P][A][od]
    float* mixed;                 // [P][A][D]
    int D, h1, h2, od;
};

// tile_row_sumsq's order (head_handle.h) over z = an - image: |anchor - d|^2 of every row (an: the anchor's D floats)
__device__ __forceinline__ float mix_row_sumsq_to(const float* buf, const float* an, int nk8) {
    const int row = threadIdx.x >> 3, part = threadIdx.x & 7;
    float s = 0.f;
    for (int k8 = part; k8 < nk8; k8 += 8) {
        const f32x4 e = *(const f32x4*)(buf + k8 * ROWP + row * 8), o = *(const f32x4*)(buf + k8 * ROWP + row * 8 + 4);
        const f32x4 a0 = *(const f32x4*)(an + k8 * 8), a1 = *(const f32x4*)(an + k8 * 8 + 4);
        const float ae[4] = {a0[0], a0[2], a1[0], a1[2]}, ao[4] = {a0[1], a0[3], a1[1], a1[3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ze = ae[j] - e[j], zo = ao[j] - o[j];
            s = fmaf(ze, ze, s);
            s = fmaf(zo, zo, s);
        }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    return s;
}

// |l - r| of the tile's 32 pairs, all D columns, into the layer-1 image (as head_fwd_kernel stages a chunk; D <= KC)
__device__ __forceinline__ void mix_stage_rows(float* buf, const HeadMix& p, const long long* s_lrow, const long long* s_rrow) {
    const int D = p.D, nk8 = D >> 3;
    for (int idx = threadIdx.x; idx < TP * nk8; idx += 256) {
        const int row = idx / nk8, k8 = idx - row * nk8;
        const long long lrow = s_lrow[row], rrow = s_rrow[row];
        const float* lp = p.L + lrow * D + k8 * 8;
        const float* rp = p.R + rrow * D + k8 * 8;
        const f32x4 l0 = *(const f32x4*)lp, l1 = *(const f32x4*)(lp + 4);
        const f32x4 r0 = *(const f32x4*)rp, r1 = *(const f32x4*)(rp + 4);
        f32x4 e, o;   // even k (h = 0) and odd k (h = 1), s = 0..3
        e[0] = fabsf(l0[0] - r0[0]); o[0] = fabsf(l0[1] - r0[1]);
        e[1] = fabsf(l0[2] - r0[2]); o[1] = fabsf(l0[3] - r0[3]);
        e[2] = fabsf(l1[0] - r1[0]); o[2] = fabsf(l1[1] - r1[1]);
        e[3] = fabsf(l1[2] - r1[2]); o[3] = fabsf(l1[3] - r1[3]);
        float* d = buf + k8 * ROWP + row * 8;
        *(f32x4*)d = e;
        *(f32x4*)(d + 4) = o;
    }
}

// layer 1 on the staged image, as head_fwd_kernel's K loop: acc must come in zeroed
template <int CT>
__device__ __forceinline__ void mix_layer1(const float* buf, const HeadMix& p, f32x16 (&acc)[CT], int colbase, int l31, int hh) {
    const int h1 = p.h1, nk8 = p.D >> 3;
    const float* wbase = p.w1p + ((size_t)colbase + l31) * 8 + hh * 4;
    for (int k8 = 0; k8 < nk8; ++k8) {
        const f32x4 a = *(const f32x4*)(buf + k8 * ROWP + l31 * 8 + hh * 4);
        f32x4 b[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) b[c] = *(const f32x4*)(wbase + ((size_t)k8 * h1 + c * 32) * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int c = 0; c < CT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[c][s], acc[c], 0, 0, 0);
    }
}

// From layer 1's accumulators to the probabilities, as head_fwd_kernel: bias and relu into the layer-2 image, layer 2 split
// over the waves, layer 3 and the softmax / sigmoid.  Every wave must be done with the layer-1 image when this is entered; the
// probabilities are in s_p (and in `out`, row stride `stride` floats, when given) once the caller has synchronised.  FIRST:
// the z1 > 0 mask of the wave's own columns is kept (bit 16 c + r of mask[c >> 1]) and u goes to LDS in the packed A-operand
// layout behind a2, as in head_egl_kernel.
template <int CT, bool FIRST>
__device__ __forceinline__ void mix_tail(float* buf, const HeadMix& p, f32x16 (&acc)[CT], unsigned (&mask)[(CT + 1) / 2], float* s_p,
                                         float* out, long long stride, long long p0, int wave, int colbase, int l31, int hh) {
    const int tid = threadIdx.x;
    const int h1 = p.h1, h2 = p.h2, od = p.od;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int col = colbase + c * 32 + l31;
        const float bb = p.b1[col];
        float* d = buf + (col >> 3) * ROWP + (col & 1) * 4 + ((col & 7) >> 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
            const float z = acc[c][r] + bb;
            d[row * 8] = fmaxf(z, 0.f);
            if (FIRST && z > 0.f) mask[c >> 1] |= 1u << ((c & 1) * 16 + r);
        }
    }
    __syncthreads();
    // ---- layer 2: wave = (column tile, K split) ----
    const int nt2 = h2 >> 5, tile = wave % nt2, ks = wave / nt2, nsplit = 4 / nt2;
    const int nk8_2 = h1 >> 3, kper = nk8_2 / nsplit;
    f32x16 acc2;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc2[i] = 0.f;
    {
        const float* w2b = p.w2p + ((size_t)tile * 32 + l31) * 8 + hh * 4;
        for (int k8 = ks * kper; k8 < (ks + 1) * kper; ++k8) {
            const f32x4 a = *(const f32x4*)(buf + k8 * ROWP + l31 * 8 + hh * 4);
            const f32x4 b = *(const f32x4*)(w2b + (size_t)k8 * h2 * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc2, 0, 0, 0);
        }
    }
    __syncthreads();
    {
        float* part = buf + ks * (TP * h2);
        const int col = tile * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
            part[row * h2 + col] = acc2[r];
        }
    }
    __syncthreads();
    float* a2 = buf + 4 * TP * 64;      // after the (at most 4 x 32 x 64) partials
    float* uimg = a2 + TP * 64;         // u, packed A-operand layout: (h2 / 8) * ROWP floats
    for (int i = tid; i < TP * h2; i += 256) {
        float s = 0.f;
        for (int z = 0; z < nsplit; ++z) s += buf[z * (TP * h2) + i];
        a2[i] = fmaxf(s + p.b2[i % h2], 0.f);
    }
    __syncthreads();
    if (FIRST) {
        for (int i = tid; i < TP * h2; i += 256) {
            const int row = i / h2, j = i - row * h2;
            const float wd = od == 2 ? p.w3[j * 2] - p.w3[j * 2 + 1] : p.w3[j];
            uimg[(j >> 3) * ROWP + row * 8 + (j & 1) * 4 + ((j & 7) >> 1)] = a2[i] > 0.f ? wd : 0.f;
        }
    }
    // ---- layer 3 (wave 0) ----
    if (tid < 2 * TP && od == 2) {
        const int row = tid >> 1, cls = tid & 1;
        float z = 0.f;
        for (int c = 0; c < h2; ++c) z = fmaf(a2[row * h2 + c], p.w3[c * 2 + cls], z);
        z += p.b3[cls];
        const float zo = __shfl_xor(z, 1, 64);
        const float m = fmaxf(z, zo);
        const float e = expf(z - m), eo = expf(zo - m);
        const float pr = e / (e + eo);
        s_p[tid] = pr;
        const long long pp = p0 + row;
        if (pp < p.P && out) out[pp * stride + cls] = pr;
    } else if (tid < TP && od == 1) {
        const int row = tid;
        float z = 0.f;
        for (int c = 0; c < h2; ++c) z = fmaf(a2[row * h2 + c], p.w3[c], z);
        z += p.b3[0];
        const float pr = 1.f / (1.f + expf(-z));
        s_p[row] = pr;
        const long long pp = p0 + row;
        if (pp < p.P && out) out[pp * stride] = pr;
    }
}

// the argmax rule on a row's probabilities in LDS: ties to class 0; one output: p > 0.5
__device__ __forceinline__ int mix_argmax(const float* s_p, int row, int od) {
    return od == 2 ? (s_p[row * 2 + 1] > s_p[row * 2] ? 1 : 0) : (s_p[row] > 0.5f ? 1 : 0);
}

constexpr int QT = 4;       // 32-column tiles of q a wave may own: ceil(16 / 4) at D = 512

// q = v W1^T on NQ 32-column tiles from column qbase: v from the image (h1 / 8 blocks), W1^T packed [h1 / 8][D][2][4]; a lane
// whose column lies past D (the last tile of a D off 32) multiplies by zero
template <int NQ>
__device__ __forceinline__ void mix_qgemm(const float* buf, const HeadMix& p, f32x16 (&q)[QT], int qbase, int l31, int hh) {
    const int D = p.D, nk8 = p.h1 >> 3;
    const float* wbase = p.w1tp + ((size_t)qbase + l31) * 8 + hh * 4;
    for (int k8 = 0; k8 < nk8; ++k8) {
        const f32x4 a = *(const f32x4*)(buf + k8 * ROWP + l31 * 8 + hh * 4);
        f32x4 b[NQ];
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
            b[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (qbase + c * 32 + l31 < D) b[c] = *(const f32x4*)(wbase + ((size_t)k8 * D + c * 32) * 8);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int c = 0; c < NQ; ++c) q[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[c][s], q[c], 0, 0, 0);
    }
}

template <int CT>
__global__ __launch_bounds__(256, 2) void head_mix_kernel(const HeadMix p) {
    extern __shared__ __attribute__((aligned(16))) float buf[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long p0 = (long long)blockIdx.x * TP;
    const int D = p.D, h1 = p.h1, h2 = p.h2, od = p.od;
    const int l31 = lane & 31, hh = lane >> 5;
    const int colbase = wave * (32 * CT);

    f32x16 acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;

    __shared__ long long s_lrow[TP], s_rrow[TP];
    __shared__ float s_p[TP * 2], s_sgn[TP], s_g[TP], s_s[TP];
    __shared__ int s_ok[TP];
    if (tid < TP) {
        long long pp = p0 + tid;
        if (pp >= p.P) pp = p.P - 1;
        s_lrow[tid] = p.li ? (long long)p.li[pp] : pp;
        s_rrow[tid] = p.ri ? (long long)p.ri[pp] : pp;
    }
    __syncthreads();
    // ---- the forward, as head_fwd_kernel ----
    mix_stage_rows(buf, p, s_lrow, s_rrow);
    __syncthreads();
    mix_layer1<CT>(buf, p, acc, colbase, l31, hh);
    __syncthreads();
    unsigned mask[(CT + 1) / 2];
#pragma unroll
    for (int i = 0; i < (CT + 1) / 2; ++i) mask[i] = 0u;
    mix_tail<CT, true>(buf, p, acc, mask, s_p, p.probs, (long long)od, p0, wave, colbase, l31, hh);
    if (!p.flip && !p.mixed_probs && !p.mixed) return;
    __syncthreads();
    // ---- v = u W2^T on the wave's own layer-1 columns, as head_egl_kernel ----
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
    {
        const float* uimg = buf + 5 * TP * 64;
        const float* wbase = p.w2tp + ((size_t)colbase + l31) * 8 + hh * 4;
        const int nk8 = h2 >> 3;
        for (int k8 = 0; k8 < nk8; ++k8) {
            const f32x4 a = *(const f32x4*)(uimg + k8 * ROWP + l31 * 8 + hh * 4);
            f32x4 b[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) b[c] = *(const f32x4*)(wbase + ((size_t)k8 * h1 + c * 32) * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[c][s], acc[c], 0, 0, 0);
        }
    }
    __syncthreads();        // u, a2 and the probabilities are read: the image's start is free, s_p is final
    int yhat = 0;           // thread t < 32: the label of row t, and the flips it collects
    unsigned flipbits = 0u;
    if (tid < TP) {
        yhat = mix_argmax(s_p, tid, od);
        s_sgn[tid] = (od == 2) == (yhat == 1) ? 1.f : -1.f;
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int col = colbase + c * 32 + l31;
        float* d = buf + (col >> 3) * ROWP + (col & 1) * 4 + ((col & 7) >> 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
            d[row * 8] = (mask[c >> 1] >> ((c & 1) * 16 + r) & 1u) ? acc[c][r] : 0.f;
        }
    }
    __syncthreads();
    // ---- q = v W1^T: wave w owns the 32-column tiles w * qt .. w * qt + nown - 1 of the D columns ----
    const int ntq = (D + 31) >> 5, qt = (ntq + 3) >> 2;
    const int nown = max(0, min(qt, ntq - wave * qt));
    const int qbase = wave * qt * 32;
    f32x16 q[QT];
#pragma unroll
    for (int c = 0; c < QT; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) q[c][i] = 0.f;
    switch (nown) {
        case 1: mix_qgemm<1>(buf, p, q, qbase, l31, hh); break;
        case 2: mix_qgemm<2>(buf, p, q, qbase, l31, hh); break;
        case 3: mix_qgemm<3>(buf, p, q, qbase, l31, hh); break;
        case 4: mix_qgemm<4>(buf, p, q, qbase, l31, hh); break;
        default: break;
    }
    __syncthreads();        // v is read: q goes into the image for its row norms
#pragma unroll
    for (int c = 0; c < QT; ++c) {
        const int col = qbase + c * 32 + l31;
        if (c < nown && col < D) {
            float* d = buf + (col >> 3) * ROWP + (col & 1) * 4 + ((col & 7) >> 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                d[row * 8] = q[c][r];
            }
        }
    }
    __syncthreads();
    {
        const float gsq = tile_row_sumsq(buf, D >> 3);
        if ((tid & 7) == 0) s_g[tid >> 3] = sqrtf(gsq);
    }
    // ---- per anchor: stage d, |anchor - d|, mix in place, the forward again ----
    for (int a = 0; a < p.A; ++a) {
        const float* an = p.anchors + (size_t)a * D;
        __syncthreads();    // the image's readers (the row norms, the last anchor's layers) are done
        mix_stage_rows(buf, p, s_lrow, s_rrow);
        __syncthreads();
        {
            const float zsq = mix_row_sumsq_to(buf, an, D >> 3);
            if ((tid & 7) == 0) {
                const int row = tid >> 3;
                const float G = s_g[row], Z = sqrtf(zsq);
                const bool ok = G != 0.f && isfinite(G) && isfinite(Z);
                s_ok[row] = ok ? 1 : 0;
                s_s[row] = ok ? s_sgn[row] * ((p.eps * Z) / G) : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < QT; ++c) {
            const int col = qbase + c * 32 + l31;
            if (c < nown && col < D) {
                const float ae = an[col];
                float* d = buf + (col >> 3) * ROWP + (col & 1) * 4 + ((col & 7) >> 1);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                    const float dd = d[row * 8];
                    const float z = ae - dd;
                    const float t = s_s[row] * q[c][r];
                    const float delta = s_ok[row] ? fminf(fmaxf(t, fminf(z, 0.f)), fmaxf(z, 0.f)) : 0.f;
                    d[row * 8] = dd + delta;
                }
            }
        }
        __syncthreads();
        if (p.mixed) {
            const int nk8 = D >> 3;
            for (int idx = tid; idx < TP * nk8; idx += 256) {
                const int row = idx / nk8, k8 = idx - row * nk8;
                const long long pp = p0 + row;
                if (pp >= p.P) continue;
                const f32x4 e = *(const f32x4*)(buf + k8 * ROWP + row * 8), o = *(const f32x4*)(buf + k8 * ROWP + row * 8 + 4);
                float* dst = p.mixed + ((size_t)pp * p.A + a) * D + k8 * 8;
                *(f32x4*)dst = f32x4{e[0], o[0], e[1], o[1]};
                *(f32x4*)(dst + 4) = f32x4{e[2], o[2], e[3], o[3]};
            }
        }
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
        mix_layer1<CT>(buf, p, acc, colbase, l31, hh);
        __syncthreads();
        mix_tail<CT, false>(buf, p, acc, mask, s_p, p.mixed_probs ? p.mixed_probs + (size_t)a * od : nullptr, (long long)p.A * od, p0,
                            wave, colbase, l31, hh);
        __syncthreads();
        if (tid < TP && mix_argmax(s_p, tid, od) != yhat) flipbits |= 1u << a;
    }
    if (tid < TP && p.flip && p0 + tid < p.P) p.flip[p0 + tid] = (uint8_t)flipbits;
}

unsigned long long g_mix_attr_done = 0;      // one bit per device: function attributes are per device
int mix_init_attrs() {
    const int dev = current_device();
    if (dev >= 0 && dev < 64 && (g_mix_attr_done >> dev & 1ull)) return ALINK_OK;
    const int lds = (int)fwd_lds_bytes(512);
    ALINK_HIP(hipFuncSetAttribute((const void*)head_mix_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ALINK_HIP(hipFuncSetAttribute((const void*)head_mix_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ALINK_HIP(hipFuncSetAttribute((const void*)head_mix_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ALINK_HIP(hipFuncSetAttribute((const void*)head_mix_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if (dev >= 0 && dev < 64) g_mix_attr_done |= 1ull << dev;
    return ALINK_OK;
}

}  // namespace

extern "C" int alink_head_feature_mix(alink_head_t* h, const float* dev_L, const float* dev_R, const int32_t* dev_li,
                                      const int32_t* dev_ri, int64_t P, const float* dev_anchors, int A, float eps, float* dev_probs,
                                      uint8_t* dev_flip, float* dev_mixed_probs, float* dev_mixed, void* stream) {
    ALINK_REQUIRE(h, ALINK_EINVAL, "NULL head");
    ALINK_REQUIRE(dev_L && dev_R, ALINK_EINVAL, "NULL feature table");
    ALINK_REQUIRE(dev_anchors, ALINK_EINVAL, "NULL anchors");
    ALINK_REQUIRE(dev_probs || dev_flip || dev_mixed_probs || dev_mixed, ALINK_EINVAL,
                  "no output asked for: dev_probs, dev_flip, dev_mixed_probs and dev_mixed are all NULL");
    ALINK_REQUIRE(P >= 0, ALINK_EINVAL, "negative pair count");
    ALINK_REQUIRE(P <= (1ll << 29) - TP, ALINK_EINVAL, "P=%lld: one launch takes at most 2^29 - 32 pairs", (long long)P);
    ALINK_REQUIRE(A >= 1 && A <= 8, ALINK_EINVAL, "A=%d anchors: 1 .. 8 (one bit of dev_flip each)", A);
    ALINK_REQUIRE(eps >= 0.f && eps <= 3.402823466e38f, ALINK_EINVAL, "eps=%g must be finite and >= 0", (double)eps);
    ALINK_REQUIRE(h->D % 8 == 0 && h->D <= KC, ALINK_EINVAL, "D=%d: the mix holds a whole row in LDS, D a multiple of 8 up to %d", h->D, KC);
    ALINK_REQUIRE(h->h1 == 128 || h->h1 == 256 || h->h1 == 384 || h->h1 == 512, ALINK_EINVAL, "h1=%d must be 128, 256, 384 or 512", h->h1);
    ALINK_REQUIRE(!h->qmode, ALINK_EINVAL, "alink_head_feature_mix is the exact float32 form: the head is in the bf16 compute mode");
    if (P == 0) return ALINK_OK;
    DeviceGuard dg(h->device);
    hipStream_t st = (hipStream_t)stream;
    int rc = mix_init_attrs();
    if (rc) return rc;
    if (!h->d_w2tp) {
        rc = h->mem.zeros((size_t)h->h1 * h->h2 * sizeof(float), (void**)&h->d_w2tp);
        if (rc) return rc;
        h->packed_dirty = true;
    }
    if (!h->d_w1tp) {
        rc = h->mem.zeros((size_t)h->D * h->h1 * sizeof(float), (void**)&h->d_w1tp);
        if (rc) return rc;
        h->packed_dirty = true;
    }
    rc = head_ensure_packed(h, st);
    if (rc) return rc;
    HeadMix p{};
    p.L = dev_L; p.R = dev_R; p.li = dev_li; p.ri = dev_ri; p.P = P;
    p.w1p = h->d_w1p; p.b1 = h->d_params + h->ob1; p.w2p = h->d_w2p; p.w2tp = h->d_w2tp; p.w1tp = h->d_w1tp;
    p.b2 = h->d_params + h->ob2; p.w3 = h->d_params + h->oW3; p.b3 = h->d_params + h->ob3;
    p.anchors = dev_anchors; p.A = A; p.eps = eps;
    p.probs = dev_probs; p.flip = dev_flip; p.mixed_probs = dev_mixed_probs; p.mixed = dev_mixed;
    p.D = h->D; p.h1 = h->h1; p.h2 = h->h2; p.od = h->od;
    const size_t lds = fwd_lds_bytes(512);
    const dim3 grid((unsigned)((P + TP - 1) / TP)), block(256);
    switch (h->h1 / 128) {
        case 1: hipLaunchKernelGGL(head_mix_kernel<1>, grid, block, lds, st, p); break;
        case 2: hipLaunchKernelGGL(head_mix_kernel<2>, grid, block, lds, st, p); break;
        case 3: hipLaunchKernelGGL(head_mix_kernel<3>, grid, block, lds, st, p); break;
        default: hipLaunchKernelGGL(head_mix_kernel<4>, grid, block, lds, st, p); break;
    }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}
