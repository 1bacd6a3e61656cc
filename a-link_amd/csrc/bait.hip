// bait.hip — BAIT batches on the device (Ash, Goel, Krishnamurthy & Kakade 2021, "Gone Fishing: Neural Active Learning with
// Fisher Embeddings"): greedy forward selection of the rows that most reduce tr(M^-1 Phi), then a backward prune.  EXTENSION
// (DESIGN.md §0, X16); include/alink_hip.h states the rule in full.  For the pair head the per-sample Fisher of the last layer
// is rank one, so a row is ONE factor f of F = h2 floats (per committee member: m factors side by side) and its score is
//     s_n = sum over blocks of  (f^T A f) / (1 + f^T B f)          B = M^-1,  A = B Phi B,  both F x F
//
// Kernels, all on the caller's stream, whose order is the ONLY ordering between workgroups (no atomics, no cooperative launch,
// no workgroup waits on another):
//   bait_factor_kernel   elementwise: f from alink_head_egl's probs and emb
//   bait_score_kernel    THE HOT ONE.  A workgroup owns BAIT_TILE = 128 rows, a wave 32 of them.  Per block the tile is staged
//                        in LDS in the packed A-operand layout of head_handle.h; [A | B] is read as the B operand from a packed
//                        global copy (m x 2 x F x F floats: 32 - 512 KB, it stays in L2, as W1 / W2 do for the head kernels);
//                        G = f A, then each accumulator row is dotted with its own f from the LDS image, the 32 column lanes
//                        meet in an xor butterfly, the same for B, then the division, the sum over blocks and the workgroup's
//                        (score, index) maximum.  No atomics, no scratch memory.
//   bait_update_kernel   one workgroup of 1,024 threads: reduces the partial maxima, records the pick, clears its free bit,
//                        float64 Woodbury step of B per block, A = B Phi B recomputed in float64 (two F^3 products, 4 x 4
//                        register tiles, operands from L2), and the packed float32 [A | B] of the next score pass
//   bait_gather_kernel / bait_compact_kernel    the backward phase's small table and the final kept rows in pick order
//
// Why A is recomputed and not carried by the rank-two identity: the state a call hands back is B alone, and a call of
// k1 + k2 forward picks must equal two chained calls bit for bit — A has to be a function of (B, Phi), not of the history.
//
// LDS of the score kernel: 4 waves x (F / 8) x ROWP floats = 65 KB at F = 128 (one workgroup per CU: 200 VGPR + 64 AGPR), 33 KB at F = 64 (three, by registers),
// 4 KB at F = 8.  The MFMA's A-operand reads (b128, lane = row) are the head kernels' conflict-free ones; the epilogue's
// scalar reads of f[row][col = lane] hit bank 8 row + 4 (col >> 3) + perm(col & 7): two lanes per bank, 16 reads per 32-column
// tile against the tile's F / 2 MFMAs of 64 cycles each — under 2 % of the loop at F = 64, left as it is.
#include "head_handle.h"

namespace alink {
namespace {

constexpr int BAIT_TILE = ALINK_BAIT_TILE;     // rows per workgroup of the score pass
constexpr int BAIT_UPD_THREADS = 1024;
constexpr int BAIT_NONE = 0x7fffffff;

struct BaitCand { float v; int i; };           // larger wins, equal -> the lower index; a NaN never enters
__device__ __forceinline__ BaitCand bait_better(BaitCand a, BaitCand b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// ---- factor -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bait_factor_kernel(const float* __restrict__ probs, const float* __restrict__ emb, long long P,
                                                          int od, int h2, float* __restrict__ f) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= P * h2) return;
    const long long n = e / h2;
    const int j = (int)(e - n * h2);
    float out = 0.f;
    if (od == 2) {
        const float q0 = probs[n * 2], q1 = probs[n * 2 + 1];
        const bool inside = q0 >= 1e-7f && q0 <= 1.f - 1e-7f && q1 >= 1e-7f && q1 <= 1.f - 1e-7f;
        const int yhat = q1 > q0 ? 1 : 0;
        const float py = yhat ? q1 : q0, pc = yhat ? q0 : q1;
        if (inside) out = emb[n * 2 * h2 + (size_t)(1 - yhat) * h2 + j] * (float)sqrt(2.0 * (double)py / (double)pc);
    } else {
        const float q = probs[n];
        const bool inside = q >= 1e-7f && q <= 1.f - 1e-7f;
        const double hit = q > 0.5f ? 1.0 : 0.0;
        if (inside) out = fabsf(emb[n * h2 + j]) * (float)(sqrt((double)q * (1.0 - (double)q)) / fabs((double)q - hit));
    }
    f[e] = out;
}

// ---- scores ---------------------------------------------------------------------------------------------------------------
// G = (tile of f) x M for one packed F x F matrix M, then q_row = sum over columns of G[row][col] f[row][col]: per lane one
// fused multiply-add per column tile in ascending order, then an xor butterfly (16, 8, 4, 2, 1) over the 32 column lanes.
template <int NT>
__device__ __forceinline__ void bait_quad(const float* __restrict__ wbuf, const float* __restrict__ mat, int F, int l31, int hh,
                                          float q[16]) {
    f32x16 acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
    const int nk8 = F >> 3;
    bool ok[NT];
    int colc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        ok[c] = c * 32 + l31 < F;
        colc[c] = ok[c] ? c * 32 + l31 : 0;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int k8 = 0; k8 < nk8; ++k8) {
        const f32x4 a = *(const f32x4*)(wbuf + k8 * ROWP + l31 * 8 + hh * 4);
        f32x4 b[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) b[c] = ok[c] ? *(const f32x4*)(mat + ((size_t)k8 * F + colc[c]) * 8 + hh * 4) : zero;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[c][s], acc[c], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int col = colc[c];
            const float fv = wbuf[(col >> 3) * ROWP + row * 8 + (col & 1) * 4 + ((col & 7) >> 1)];
            s = fmaf(acc[c][r], ok[c] ? fv : 0.f, s);
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        q[r] = s;
    }
}

template <int NT>
__global__ __launch_bounds__(256) void bait_score_kernel(const float* __restrict__ f, long long N, int F, int m, const float* __restrict__ AB,
                                                         const uint8_t* __restrict__ dev_free, int sign, float* __restrict__ scores_out,
                                                         BaitCand* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float bait_lds[];
    __shared__ BaitCand s_best[4];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk8 = F >> 3, ld = m * F;
    const long long n0 = (long long)blockIdx.x * BAIT_TILE;
    float* wbuf = bait_lds + (size_t)wave * nk8 * ROWP;
    float score[16];
    bool skip[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { score[r] = 0.f; skip[r] = false; }
    for (int j = 0; j < m; ++j) {
        if (j) __syncthreads();                            // every wave is done with the previous block's image
        for (int idx = tid; idx < BAIT_TILE * nk8; idx += 256) {
            const int row = idx / nk8, k8 = idx - row * nk8;
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (n0 + row < N) {
                const float* src = f + (n0 + row) * ld + (size_t)j * F + k8 * 8;
                v0 = *(const f32x4*)src;
                v1 = *(const f32x4*)(src + 4);
            }
            f32x4 e, o;                                    // even k (h = 0) and odd k (h = 1), s = 0..3
            e[0] = v0[0]; o[0] = v0[1]; e[1] = v0[2]; o[1] = v0[3];
            e[2] = v1[0]; o[2] = v1[1]; e[3] = v1[2]; o[3] = v1[3];
            float* d = bait_lds + ((size_t)(row >> 5) * nk8 + k8) * ROWP + (row & 31) * 8;
            *(f32x4*)d = e;
            *(f32x4*)(d + 4) = o;
        }
        __syncthreads();
        float qa[16], qb[16];
        const float* mat = AB + (size_t)j * 2 * F * F;
        bait_quad<NT>(wbuf, mat, F, l31, hh, qa);
        bait_quad<NT>(wbuf, mat + (size_t)F * F, F, l31, hh, qb);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float den = sign > 0 ? 1.f + qb[r] : qb[r] - 1.f;
            const float term = qa[r] / den;
            score[r] = j ? score[r] + term : term;
            if (sign < 0 && qb[r] >= 1.f) skip[r] = true;
        }
    }
    BaitCand best{-INFINITY, BAIT_NONE};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long n = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        const float s = skip[r] ? __builtin_nanf("") : score[r];
        if (n < N) {
            if (scores_out && l31 == r) scores_out[n] = s;
            if (dev_free[n] && s == s) best = bait_better(best, BaitCand{s, (int)n});
        }
    }
    {
        BaitCand other;
        other.v = __shfl_xor(best.v, 32, 64);
        other.i = __shfl_xor(best.i, 32, 64);
        best = bait_better(best, other);
    }
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = bait_better(best, s_best[w]);
        partial[blockIdx.x] = best;
    }
}

// ---- the one-workgroup step -------------------------------------------------------------------------------------------------
// Z = X^T Y for F x F float64 matrices in global memory (X symmetric in every use: row k of X stands for its column k), 4 x 4
// register tiles, k ascending, one fused multiply-add per term.  `outd` (float64, row-major) and / or `outp` (float32, the packed
// B-operand layout of the score pass) receive Z.
__device__ __forceinline__ void bait_matmul(const double* __restrict__ X, const double* __restrict__ Y, int F, double* __restrict__ outd,
                                            float* __restrict__ outp) {
    const int tw = F >> 2;
    for (int t = threadIdx.x; t < tw * tw; t += BAIT_UPD_THREADS) {
        const int i0 = (t / tw) * 4, j0 = (t % tw) * 4;
        double z[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) z[a][b] = 0.0;
        for (int k = 0; k < F; ++k) {
            double x[4], y[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { x[a] = X[(size_t)k * F + i0 + a]; y[a] = Y[(size_t)k * F + j0 + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) z[a][b] = fma(x[a], y[b], z[a][b]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = i0 + a, j = j0 + b;
                if (outd) outd[(size_t)i * F + j] = z[a][b];
                if (outp) outp[((size_t)(i >> 3) * F + j) * 8 + (i & 1) * 4 + ((i & 7) >> 1)] = (float)z[a][b];
            }
    }
}

// step < 0: no pick, only A = B Phi B and the packed images (the start of a call)
__global__ __launch_bounds__(BAIT_UPD_THREADS) void bait_update_kernel(const BaitCand* __restrict__ partial, int nparts, const float* __restrict__ f,
                                                                       int F, int m, const double* __restrict__ Phi, double* __restrict__ B,
                                                                       double* __restrict__ C, float* __restrict__ AB, uint8_t* __restrict__ dev_free,
                                                                       int sign, int step, int32_t* __restrict__ idx_out, float* __restrict__ score_out,
                                                                       int nrows, int k_keep) {
    __shared__ BaitCand s_cand[BAIT_UPD_THREADS / 64];
    __shared__ int s_kept[BAIT_UPD_THREADS / 64];
    __shared__ double s_f[128], s_w[128];
    const int tid = threadIdx.x;
    int pick = -1;
    if (sign < 0) {                                        // the prune runs only WHILE more than k_keep picks are kept
        int kept = 0;
        for (int i = tid; i < nrows; i += BAIT_UPD_THREADS) kept += dev_free[i] != 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
        if ((tid & 63) == 0) s_kept[tid >> 6] = kept;
        __syncthreads();
        kept = 0;
        for (int w = 0; w < BAIT_UPD_THREADS / 64; ++w) kept += s_kept[w];
        if (kept <= k_keep) return;                        // (uniform over the workgroup) fewer picks than k_forward were found
    }
    if (step >= 0) {
        BaitCand c{-INFINITY, BAIT_NONE};
        for (int i = tid; i < nparts; i += BAIT_UPD_THREADS) c = bait_better(c, partial[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            BaitCand b;
            b.v = __shfl_xor(c.v, o, 64);
            b.i = __shfl_xor(c.i, o, 64);
            c = bait_better(c, b);
        }
        if ((tid & 63) == 0) s_cand[tid >> 6] = c;
        __syncthreads();
        c = s_cand[0];
        for (int w = 1; w < BAIT_UPD_THREADS / 64; ++w) c = bait_better(c, s_cand[w]);
        pick = c.i != BAIT_NONE ? c.i : -1;
        if (tid == 0) {
            idx_out[step] = pick;
            score_out[step] = pick >= 0 ? c.v : __builtin_nanf("");
            if (pick >= 0) dev_free[pick] = 0;
        }
        if (pick < 0) return;                              // nothing to take (uniform over the workgroup): the state stays
    }
    const int ld = m * F;
    for (int j = 0; j < m; ++j) {
        double* Bj = B + (size_t)j * F * F;
        if (step >= 0) {
            __syncthreads();
            if (tid < F) s_f[tid] = (double)f[(size_t)pick * ld + (size_t)j * F + tid];
            __syncthreads();
            if (tid < F) {                                 // w = B f: row k of the symmetric B stands for its column, k ascending
                double w = 0.0;
                for (int k = 0; k < F; ++k) w = fma(Bj[(size_t)k * F + tid], s_f[k], w);
                s_w[tid] = w;
            }
            __syncthreads();
            double fw = 0.0;
            for (int k = 0; k < F; ++k) fw = fma(s_f[k], s_w[k], fw);
            const double den = sign > 0 ? 1.0 + fw : fw - 1.0;     // backward: B + w w^T / (1 - f^T w)
            for (int e = tid; e < F * F; e += BAIT_UPD_THREADS) Bj[e] -= (s_w[e / F] * s_w[e % F]) / den;
        }
        __syncthreads();                                   // B's new values are seen by the whole workgroup
        bait_matmul(Phi + (size_t)j * F * F, Bj, F, C, nullptr);                  // C = Phi B
        __syncthreads();
        bait_matmul(Bj, C, F, nullptr, AB + (size_t)j * 2 * F * F);               // A = B C -> packed float32
        for (int e = tid; e < F * F; e += BAIT_UPD_THREADS) {
            const int i = e / F, c = e % F;
            AB[(size_t)j * 2 * F * F + (size_t)F * F + ((size_t)(i >> 3) * F + c) * 8 + (i & 1) * 4 + ((i & 7) >> 1)] = (float)Bj[e];
        }
        __syncthreads();                                   // C is free again
    }
}

// the backward phase's table: row t = the factor row of forward pick t (zeros and not kept where the pick is -1)
__global__ __launch_bounds__(256) void bait_gather_kernel(const float* __restrict__ f, int ld, const int32_t* __restrict__ idx, int k,
                                                          float* __restrict__ table, uint8_t* __restrict__ keep) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)k * ld) return;
    const int t = (int)(e / ld), c = (int)(e - (long long)t * ld);
    const int n = idx[t];
    table[e] = n >= 0 ? f[(size_t)n * ld + c] : 0.f;
    if (c == 0) keep[t] = n >= 0;
}

// the first k_keep kept picks in pick order; every other pick is free again
__global__ __launch_bounds__(256) void bait_compact_kernel(const int32_t* __restrict__ idx, const float* __restrict__ score,
                                                           const uint8_t* __restrict__ keep, int k, int k_keep, uint8_t* __restrict__ dev_free,
                                                           int32_t* __restrict__ idx_out, float* __restrict__ score_out) {
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < k; t0 += 256) {
        const int t = t0 + tid;
        const bool kept = t < k && keep[t] != 0;
        const unsigned long long bal = __ballot(kept);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int pos = s_base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += s_wave[w];
        if (t < k) {
            if (kept && pos < k_keep) {
                idx_out[pos] = idx[t];
                score_out[pos] = score[t];
            } else if (idx[t] >= 0) {
                dev_free[idx[t]] = 1;
            }
        }
        __syncthreads();
        if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    for (int p = s_base + tid; p < k_keep; p += 256) {
        idx_out[p] = -1;
        score_out[p] = __builtin_nanf("");
    }
}

size_t bait_align(size_t b) { return (b + 255) & ~(size_t)255; }
size_t bait_score_lds(int F) { return (size_t)4 * (F >> 3) * ROWP * sizeof(float); }
int bait_parts(long long N) { return (int)((N + BAIT_TILE - 1) / BAIT_TILE); }

bool bait_shape_ok(int F, int m) { return F >= 8 && F <= 128 && F % 8 == 0 && m >= 1 && m <= 8 && m * F <= 512; }

void bait_launch_scores(const float* f, long long N, int F, int m, const float* AB, const uint8_t* dev_free, int sign, float* scores,
                        BaitCand* partial, hipStream_t st) {
    const dim3 grid((unsigned)bait_parts(N)), block(256);
    const size_t lds = bait_score_lds(F);
    switch ((F + 31) >> 5) {
    case 1: hipLaunchKernelGGL(bait_score_kernel<1>, grid, block, lds, st, f, N, F, m, AB, dev_free, sign, scores, partial); break;
    case 2: hipLaunchKernelGGL(bait_score_kernel<2>, grid, block, lds, st, f, N, F, m, AB, dev_free, sign, scores, partial); break;
    case 3: hipLaunchKernelGGL(bait_score_kernel<3>, grid, block, lds, st, f, N, F, m, AB, dev_free, sign, scores, partial); break;
    default: hipLaunchKernelGGL(bait_score_kernel<4>, grid, block, lds, st, f, N, F, m, AB, dev_free, sign, scores, partial); break;
    }
}

// the score kernel's dynamic LDS goes beyond the 64 KB a kernel gets without asking, at F = 128
int bait_set_attributes() {
    const int bytes = (int)bait_score_lds(128);
    ALINK_HIP(hipFuncSetAttribute((const void*)bait_score_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    ALINK_HIP(hipFuncSetAttribute((const void*)bait_score_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    ALINK_HIP(hipFuncSetAttribute((const void*)bait_score_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    ALINK_HIP(hipFuncSetAttribute((const void*)bait_score_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return ALINK_OK;
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

int alink_fisher_factor(const float* dev_probs, const float* dev_emb, int64_t P, int od, int h2, float* dev_f, void* stream) {
    ALINK_REQUIRE(dev_probs && dev_emb && dev_f, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(P >= 0 && P < (1ll << 31), ALINK_EINVAL, "P=%lld outside 0..2^31-1", (long long)P);
    ALINK_REQUIRE(od == 1 || od == 2, ALINK_EINVAL, "od=%d: one or two outputs", od);
    ALINK_REQUIRE(h2 >= 1 && h2 <= 4096, ALINK_EINVAL, "h2=%d outside 1..4096", h2);
    if (P == 0) return ALINK_OK;
    DeviceGuard dg(device_of_pointer(dev_f));
    const long long total = (long long)P * h2;
    hipLaunchKernelGGL(bait_factor_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dev_probs, dev_emb,
                       (long long)P, od, h2, dev_f);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

int alink_bait_scores(const float* dev_f, int64_t N, int F, int m, const float* dev_AB, const uint8_t* dev_free, int sign,
                      float* dev_scores, void* dev_partial_best, void* stream) {
    ALINK_REQUIRE(dev_f && dev_AB && dev_free && dev_partial_best, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(bait_shape_ok(F, m), ALINK_EINVAL, "F=%d, m=%d: F a multiple of 8 in 8..128, m in 1..8, m F <= 512", F, m);
    ALINK_REQUIRE(sign == 1 || sign == -1, ALINK_EINVAL, "sign=%d: +1 forward, -1 backward", sign);
    ALINK_REQUIRE((((uintptr_t)dev_f | (uintptr_t)dev_AB) & 15) == 0, ALINK_EINVAL, "the row table and the packed matrices must be 16-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_f));
    if (int rc = bait_set_attributes()) return rc;
    bait_launch_scores(dev_f, N, F, m, dev_AB, dev_free, sign, dev_scores, (BaitCand*)dev_partial_best, (hipStream_t)stream);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

size_t alink_bait_select_scratch_bytes(int64_t N, int F, int m, int k_forward) {
    if (N < 1 || k_forward < 1 || !bait_shape_ok(F, m)) return 0;
    const long long big = N > k_forward ? N : k_forward;
    return bait_align((size_t)bait_parts(big) * sizeof(BaitCand)) + bait_align((size_t)F * F * sizeof(double))
           + bait_align((size_t)m * 2 * F * F * sizeof(float)) + 2 * bait_align((size_t)k_forward * 4)
           + bait_align((size_t)k_forward * m * F * sizeof(float)) + bait_align((size_t)k_forward) + 256;
}

int alink_bait_select(const float* dev_f, int64_t N, int F, int m, const double* dev_Phi, double* dev_B, uint8_t* dev_free,
                      int k_forward, int k_keep, int32_t* dev_idx, float* dev_score, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_f && dev_Phi && dev_B && dev_free && dev_idx && dev_score && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(bait_shape_ok(F, m), ALINK_EINVAL, "F=%d, m=%d: F a multiple of 8 in 8..128, m in 1..8, m F <= 512", F, m);
    ALINK_REQUIRE(k_keep >= 1 && k_forward >= k_keep && (int64_t)k_forward <= N, ALINK_EINVAL, "k_forward=%d, k_keep=%d: 1 <= k_keep <= k_forward <= N",
                  k_forward, k_keep);
    ALINK_REQUIRE(((uintptr_t)dev_f & 15) == 0, ALINK_EINVAL, "the row table must be 16-byte aligned");
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_f));
    if (int rc = bait_set_attributes()) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)dev_scratch;
    const long long big = N > k_forward ? N : k_forward;
    BaitCand* partial = (BaitCand*)s;            s += bait_align((size_t)bait_parts(big) * sizeof(BaitCand));
    double* C = (double*)s;                      s += bait_align((size_t)F * F * sizeof(double));
    float* AB = (float*)s;                       s += bait_align((size_t)m * 2 * F * F * sizeof(float));
    int32_t* idx_fwd = (int32_t*)s;              s += bait_align((size_t)k_forward * 4);
    float* score_fwd = (float*)s;                s += bait_align((size_t)k_forward * 4);
    float* table = (float*)s;                    s += bait_align((size_t)k_forward * m * F * sizeof(float));
    uint8_t* keep = (uint8_t*)s;                 s += bait_align((size_t)k_forward);
    int32_t* rem = (int32_t*)s;
    const bool prune = k_keep < k_forward;
    int32_t* fi = prune ? idx_fwd : dev_idx;
    float* fs = prune ? score_fwd : dev_score;
    const dim3 one(1), upd(BAIT_UPD_THREADS);
    hipLaunchKernelGGL(bait_update_kernel, one, upd, 0, st, (const BaitCand*)nullptr, 0, dev_f, F, m, dev_Phi, dev_B, C, AB, dev_free, 1, -1, fi, fs, 0, 0);
    for (int t = 0; t < k_forward; ++t) {
        bait_launch_scores(dev_f, N, F, m, AB, dev_free, 1, nullptr, partial, st);
        hipLaunchKernelGGL(bait_update_kernel, one, upd, 0, st, (const BaitCand*)partial, bait_parts(N), dev_f, F, m, dev_Phi, dev_B, C, AB, dev_free, 1,
                           t, fi, fs, 0, 0);
    }
    if (prune) {
        const int ld = m * F;
        const long long total = (long long)k_forward * ld;
        hipLaunchKernelGGL(bait_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dev_f, ld, (const int32_t*)idx_fwd, k_forward,
                           table, keep);
        for (int t = 0; t < k_forward - k_keep; ++t) {
            bait_launch_scores(table, k_forward, F, m, AB, keep, -1, nullptr, partial, st);
            hipLaunchKernelGGL(bait_update_kernel, one, upd, 0, st, (const BaitCand*)partial, bait_parts(k_forward), (const float*)table, F, m, dev_Phi,
                               dev_B, C, AB, keep, -1, 0, rem, (float*)rem + 1, k_forward, k_keep);   // (what was removed is of no use to the caller)
        }
        hipLaunchKernelGGL(bait_compact_kernel, one, dim3(256), 0, st, (const int32_t*)idx_fwd, (const float*)score_fwd, (const uint8_t*)keep, k_forward,
                           k_keep, dev_free, dev_idx, dev_score);
    }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
