// egl.hip — expected gradient length (Settles, Craven & Ray 2008) and the last layer's gradient embedding (BADGE: Ash et
// al. 2020) of a pool of pairs, through the pair head of head.hip.  EXTENSION: the reference takes its
// strategies from modAL, which scores a pair from the head's output probabilities alone.
//
// For one pair x, l_c(x) is the loss alink_head_train_step computes on the batch {x} with target class c and sample weight 1
// (Keras' binary_crossentropy as restated at the top of head.hip), g_c(x) its gradient over all six parameter tensors, and
//     EGL(x) = sum over c in {0, 1} of P(c | x) |g_c(x)|_2.
// The per-sample gradient of a dense layer is the outer product (input) x (dz), so its norm is |input| |dz| and no weight
// gradient is ever formed.  With d = |l - r|, a1 = relu(z1), a2 = relu(z2), dz3 = p - y for both head types, and
//     u = (W3[:,0] - W3[:,1]) . [z2 > 0]   (od = 2, n3 = 2)      u = W3[:,0] . [z2 > 0]   (od = 1, n3 = 1)
//     v = (u W2^T) . [z1 > 0]
//     G^2 = n3 (|a2|^2 + 1) + |u|^2 (|a1|^2 + 1) + |v|^2 (|d|^2 + 1)
//     EGL = 2 p0 p1 sqrt(G^2)  (od = 2)        EGL = 2 p (1 - p) sqrt(G^2)  (od = 1)
// and exactly 0 on a row with an output outside [1e-7, 1 - 1e-7]: the clip kills the step's gradient there.
//
// head_egl_kernel<CT> is head_fwd_kernel<CT> (32 pairs per workgroup, v_mfma_f32_32x32x2_f32, |l - r| staged by index from the two
// feature tables) with the same packed weights, k order, layer-2 split, sum order and softmax expression, so its probabilities
// are the forward's bit for bit.  On top of it: the squared row norms of d, a1 and v are read off the LDS image each of them is
// staged in (tile_row_sumsq), the z1 > 0 mask of a wave's own columns is kept as 16 CT bits per lane, u goes to LDS in the
// packed A-operand layout and a third MFMA GEMM (M = 32 pairs, N = h1, K = h2) forms v from the packed W2^T copy.  Every sum
// runs in an order fixed by (D, h1, h2) alone: no atomics, and a pair's outputs do not depend on P, on its tile or on its
// place in the tile.
#include "head_handle.h"

using namespace alink;

namespace {

struct HeadEgl {
    const float *L, *R;
    const int32_t *li, *ri;
    long long P;
    const float *w1p, *b1, *w2p, *w2tp, *b2, *w3, *b3;
    float *egl, *probs, *emb;     // [P], [P][od], [P][od * h2]; each may be nullptr
    int D, h1, h2, od;
    int accumulate;               // add to the egl already there (committee member > 0)
    float final_div;              // > 0: divide by it after adding (last committee member)
};

template <int CT>
__global__ __launch_bounds__(256, 2) void head_egl_kernel(const HeadEgl p) {
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
    __shared__ float s_p[TP * 2], s_a2sq[TP], s_usq[TP];
    if (tid < TP) {
        long long pp = p0 + tid;
        if (pp >= p.P) pp = p.P - 1;
        s_lrow[tid] = p.li ? (long long)p.li[pp] : pp;
        s_rrow[tid] = p.ri ? (long long)p.ri[pp] : pp;
    }
    float dsq = 0.f;        // |d|^2 of row tid >> 3, chunk after chunk
    // ---- layer 1, as head_fwd_kernel ----
    for (int k0 = 0; k0 < D; k0 += KC) {
        const int kc = min(KC, D - k0), nk8 = kc >> 3;
        __syncthreads();
        for (int idx = tid; idx < TP * nk8; idx += 256) {
            const int row = idx / nk8, k8 = idx - row * nk8;
            const long long lrow = s_lrow[row], rrow = s_rrow[row];
            const float* lp = p.L + lrow * D + k0 + k8 * 8;
            const float* rp = p.R + rrow * D + k0 + k8 * 8;
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
        __syncthreads();
        dsq += tile_row_sumsq(buf, nk8);
        const float* wbase = p.w1p + ((size_t)(k0 >> 3) * h1 + colbase + l31) * 8 + hh * 4;
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
    __syncthreads();
    // A1 = relu(Z1 + b1) -> LDS in the packed A-operand layout of layer 2; bit 16 c + r of `mask`: z1 > 0 at (row of r, column c)
    unsigned mask[(CT + 1) / 2];
#pragma unroll
    for (int i = 0; i < (CT + 1) / 2; ++i) mask[i] = 0u;
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
            if (z > 0.f) mask[c >> 1] |= 1u << ((c & 1) * 16 + r);
        }
    }
    __syncthreads();
    const float a1sq = tile_row_sumsq(buf, h1 >> 3);
    // ---- layer 2: wave = (column tile, K split), as head_fwd_kernel ----
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
    // ---- layer 3 (wave 0, as head_fwd_kernel), |a2|^2 and |u|^2 (wave 1), u -> LDS (everyone) ----
    for (int i = tid; i < TP * h2; i += 256) {
        const int row = i / h2, j = i - row * h2;
        const float wd = od == 2 ? p.w3[j * 2] - p.w3[j * 2 + 1] : p.w3[j];
        uimg[(j >> 3) * ROWP + row * 8 + (j & 1) * 4 + ((j & 7) >> 1)] = a2[i] > 0.f ? wd : 0.f;
    }
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
        if (pp < p.P && p.probs) p.probs[pp * 2 + cls] = pr;
    } else if (tid < TP && od == 1) {
        const int row = tid;
        float z = 0.f;
        for (int c = 0; c < h2; ++c) z = fmaf(a2[row * h2 + c], p.w3[c], z);
        z += p.b3[0];
        const float pr = 1.f / (1.f + expf(-z));
        s_p[row] = pr;
        const long long pp = p0 + row;
        if (pp < p.P && p.probs) p.probs[pp] = pr;
    }
    if (wave == 1) {
        // lane = (row, half): the half's columns in ascending order, then the two halves
        const int row = lane >> 1, j0 = (lane & 1) * (h2 >> 1);
        float sa = 0.f, su = 0.f;
        for (int j = j0; j < j0 + (h2 >> 1); ++j) {
            const float a = a2[row * h2 + j];
            const float wd = od == 2 ? p.w3[j * 2] - p.w3[j * 2 + 1] : p.w3[j];
            const float u = a > 0.f ? wd : 0.f;
            sa = fmaf(a, a, sa);
            su = fmaf(u, u, su);
        }
        sa += __shfl_xor(sa, 1, 64);
        su += __shfl_xor(su, 1, 64);
        if ((lane & 1) == 0) { s_a2sq[row] = sa; s_usq[row] = su; }
    }
    __syncthreads();
    // ---- gradient embedding: emb[c * h2 + j] = (p_c - [c = yhat]) a2[j], zero on a saturated row ----
    if (p.emb) {
        const int w = od * h2;
        for (int i = tid; i < TP * w; i += 256) {
            const int row = i / w, rem = i - row * w, c = rem / h2, j = rem - c * h2;
            const long long pp = p0 + row;
            if (pp >= p.P) continue;
            float pc, dz;
            bool inside;
            if (od == 2) {
                const float q0 = s_p[row * 2], q1 = s_p[row * 2 + 1];
                const int yhat = q1 > q0 ? 1 : 0;
                pc = c ? q1 : q0;
                dz = pc - (c == yhat ? 1.f : 0.f);
                inside = q0 >= 1e-7f && q0 <= 1.f - 1e-7f && q1 >= 1e-7f && q1 <= 1.f - 1e-7f;
            } else {
                pc = s_p[row];
                dz = pc - (pc > 0.5f ? 1.f : 0.f);
                inside = pc >= 1e-7f && pc <= 1.f - 1e-7f;
            }
            p.emb[pp * w + rem] = inside ? dz * a2[row * h2 + j] : 0.f;
        }
    }
    if (!p.egl) return;
    // ---- v = u W2^T on the wave's own layer-1 columns ----
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
    {
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
    __syncthreads();        // u, a2 and the probabilities' readers are done: the image's start is free
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
    const float vsq = tile_row_sumsq(buf, h1 >> 3);
    if ((tid & 7) == 0) {
        const int row = tid >> 3;
        const long long pp = p0 + row;
        if (pp < p.P) {
            float pq;
            bool inside;
            if (od == 2) {
                const float q0 = s_p[row * 2], q1 = s_p[row * 2 + 1];
                pq = q0 * q1;
                inside = q0 >= 1e-7f && q0 <= 1.f - 1e-7f && q1 >= 1e-7f && q1 <= 1.f - 1e-7f;
            } else {
                const float q = s_p[row];
                pq = q * (1.f - q);
                inside = q >= 1e-7f && q <= 1.f - 1e-7f;
            }
            const float g2 = (float)od * (s_a2sq[row] + 1.f) + s_usq[row] * (a1sq + 1.f) + vsq * (dsq + 1.f);
            float e = inside ? 2.f * pq * sqrtf(g2) : 0.f;
            if (p.accumulate) e += p.egl[pp];
            if (p.final_div > 0.f) e = e / p.final_div;
            p.egl[pp] = e;
        }
    }
}

unsigned long long g_egl_attr_done = 0;      // one bit per device: function attributes are per device
int egl_init_attrs() {
    const int dev = current_device();
    if (dev >= 0 && dev < 64 && (g_egl_attr_done >> dev & 1ull)) return ALINK_OK;
    const int lds = (int)fwd_lds_bytes(512);
    ALINK_HIP(hipFuncSetAttribute((const void*)head_egl_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ALINK_HIP(hipFuncSetAttribute((const void*)head_egl_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ALINK_HIP(hipFuncSetAttribute((const void*)head_egl_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ALINK_HIP(hipFuncSetAttribute((const void*)head_egl_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if (dev >= 0 && dev < 64) g_egl_attr_done |= 1ull << dev;
    return ALINK_OK;
}

}  // namespace

extern "C" int alink_head_egl(alink_head_t* h, const float* dev_L, const float* dev_R, const int32_t* dev_li, const int32_t* dev_ri,
                              int64_t P, int accumulate, float final_div, float* dev_egl, float* dev_probs, float* dev_emb,
                              void* stream) {
    ALINK_REQUIRE(h, ALINK_EINVAL, "NULL head");
    ALINK_REQUIRE(dev_L && dev_R, ALINK_EINVAL, "NULL feature table");
    ALINK_REQUIRE(dev_egl || dev_probs || dev_emb, ALINK_EINVAL, "no output asked for: dev_egl, dev_probs and dev_emb are all NULL");
    ALINK_REQUIRE(P >= 0, ALINK_EINVAL, "negative pair count");
    ALINK_REQUIRE(!accumulate || dev_egl, ALINK_EINVAL, "accumulate acts on dev_egl, which is NULL");
    ALINK_REQUIRE(!h->qmode, ALINK_EINVAL, "alink_head_egl is the exact float32 form: the head is in the bf16 compute mode");
    ALINK_REQUIRE(P <= (1ll << 29) - TP, ALINK_EINVAL, "P=%lld: one launch takes at most 2^29 - 32 pairs", (long long)P);
    if (P == 0) return ALINK_OK;
    DeviceGuard dg(h->device);
    hipStream_t st = (hipStream_t)stream;
    int rc = egl_init_attrs();
    if (rc) return rc;
    if (!h->d_w2tp) {
        rc = h->mem.zeros((size_t)h->h1 * h->h2 * sizeof(float), (void**)&h->d_w2tp);
        if (rc) return rc;
        h->packed_dirty = true;
    }
    rc = head_ensure_packed(h, st);
    if (rc) return rc;
    HeadEgl p{};
    p.L = dev_L; p.R = dev_R; p.li = dev_li; p.ri = dev_ri; p.P = P;
    p.w1p = h->d_w1p; p.b1 = h->d_params + h->ob1; p.w2p = h->d_w2p; p.w2tp = h->d_w2tp; p.b2 = h->d_params + h->ob2;
    p.w3 = h->d_params + h->oW3; p.b3 = h->d_params + h->ob3;
    p.egl = dev_egl; p.probs = dev_probs; p.emb = dev_emb;
    p.D = h->D; p.h1 = h->h1; p.h2 = h->h2; p.od = h->od; p.accumulate = accumulate; p.final_div = final_div;
    const size_t lds = fwd_lds_bytes(h->h1);
    const dim3 grid((unsigned)((P + TP - 1) / TP)), block(256);
    switch (h->h1 / 128) {
        case 1: hipLaunchKernelGGL(head_egl_kernel<1>, grid, block, lds, st, p); break;
        case 2: hipLaunchKernelGGL(head_egl_kernel<2>, grid, block, lds, st, p); break;
        case 3: hipLaunchKernelGGL(head_egl_kernel<3>, grid, block, lds, st, p); break;
        case 4: hipLaunchKernelGGL(head_egl_kernel<4>, grid, block, lds, st, p); break;
        default: set_error("h1=%d unsupported", h->h1); return ALINK_EINVAL;
    }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}
