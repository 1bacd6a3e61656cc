// batch.hip — ranked batch-mode query selection on device (modAL.batch: Cardoso et al. 2017, "Ranked batch-mode active
// learning"), a pure streaming pass per pick: HBM-bound vector-ALU work, no MFMA.
//
// The rule (include/alink_hip.h states it in full): d2[n] = the squared Euclidean distance of pool row n to the nearest
// labelled row or earlier pick; pick t maximises alpha_t (1 - 1 / (1 + sqrt(d2))) + (1 - alpha_t) u over the rows not yet
// picked, ties to the lower index; then d2 takes the new pick into account.  modAL does this on the host with one full
// pairwise_distances_argmin_min per pick.
//
// Launches, all on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative launch, no
// grid barrier, no workgroup waits on another):
//   rb_init_kernel     d2[n] = min_m |x_n - z_m|^2: a workgroup owns 32 pool rows, the labelled rows pass through LDS in tiles,
//                      a wave takes 4 pool rows x 4 labelled rows at a time
//   rb_step_kernel x k one per pick, one fixed grid.  Prologue: EVERY workgroup reduces the previous launch's per-workgroup
//                      partials to the previous pick (workgroup 0 records it) and puts that row into LDS; then a wave walks
//                      its rows two at a time: d2 = min(d2, |x - pick|^2), the score, the wave's best; last the workgroup's
//                      partial.  Partials are double-buffered by the parity of t: launch t reads (t - 1) & 1 and writes t & 1,
//                      so no workgroup's write can meet another's prologue read.
//   rb_finish_kernel   reduces the last partials to the last pick
// A picked row is marked by d2 = -1 (a squared distance is never negative): no second array.
//
// One summation order for every squared distance, a function of D alone: batch_rows.h states it and holds the code.
#include "batch_rows.h"

namespace alink {
namespace {

constexpr int RB_MAX_GRID = 2048;          // workgroups of the step kernel (eight per CU, all resident) = partials every prologue reduces
constexpr int RB_PASS_ROWS = 2;            // step kernel: neighbouring rows per wave and pass
constexpr int RB_NONE = 0x7fffffff;        // index of a candidate that has seen no score at all

// (score, index): b replaces a when strictly larger, or equal with the lower index — a total order, so the maximum does
// not depend on the order the candidates meet in.  A NaN compares false both ways and never enters.
struct RbCand { float v; int i; };
__device__ __forceinline__ RbCand rb_better(RbCand a, RbCand b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ RbCand rb_wave_max(RbCand a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        RbCand b;
        b.v = __shfl_xor(a.v, o, 64);
        b.i = __shfl_xor(a.i, o, 64);
        a = rb_better(a, b);
    }
    return a;
}

// alpha (1 - 1 / (1 + sqrt(d2))) + (1 - alpha) u: every operation rounded once, sqrt and division correctly rounded (the
// compiler's default for float), no product contracted into the sum
__device__ __forceinline__ float rb_score(float d2, float u, float alpha, float one_minus_alpha) {
#pragma clang fp contract(off)
    const float d = sqrtf(d2);
    const float s = 1.f / (1.f + d);
    const float apart = 1.f - s;
    const float a = alpha * apart;
    const float b = one_minus_alpha * u;
    return a + b;
}

// row `src` of the pool -> LDS, zero-padded to Dp = D rounded up to a multiple of 4
template <bool PAIR>
__device__ __forceinline__ void rb_stage_row(const RbRow& src, int D, int Dp, float* dst) {
    for (int e = threadIdx.x; e < Dp; e += 256) dst[e] = e < D ? rb_elem<PAIR>(src, e) : 0.f;
}

// rb_block_pair_sums leaves lane L with |x_a - z_b|^2 for a = L >> 4, b = (L >> 2) & 3; the minimum over b follows, so L returns
// min_b |x_a - z_b|^2 for a = L >> 4.
__device__ __forceinline__ float rb_block_row_minima(float (&s)[16], int lane) {
    float v = rb_block_pair_sums(s, lane);
    v = fminf(v, __shfl_xor(v, 8, 64));
    v = fminf(v, __shfl_xor(v, 4, 64));
    return v;
}

// A wave owns RB_WG_ROWS / 4 pool rows and takes them four at a time against four labelled rows of the LDS tile: every quad
// read from LDS meets four pool rows, every pool quad four labelled rows.  SHORT (D <= 512, at most two quads per lane): the
// four pool rows stay in registers while the whole tile passes; otherwise, any D, they are read again for every block.
template <bool PAIR, bool VEC, bool SHORT>
__global__ __launch_bounds__(256) void rb_init_kernel(const RbRows t, long long N, const float* __restrict__ labeled, long long M,
                                                      int tile_rows, float* __restrict__ d2) {
    __shared__ __attribute__((aligned(16))) float tile[RB_MAX_D];
    constexpr int RW = RB_WG_ROWS / 4;
    const int D = t.D, Dp = (D + 3) & ~3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * RB_WG_ROWS + wave * RW;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float best = INFINITY;                                 // lane L: the minimum of the wave's row 4 (L & 15) + (L >> 4)
    for (long long m0 = 0; m0 < M; m0 += tile_rows) {
        const int tm = (int)(M - m0 < tile_rows ? M - m0 : tile_rows);
        __syncthreads();                                   // the previous tile has been consumed
        for (int r = wave; r < tm; r += 4) {               // a wave copies a labelled row
            const float* src = labeled + (size_t)(m0 + r) * D;
            for (int c = lane; c < Dp; c += 64) tile[r * Dp + c] = c < D ? src[c] : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int g = 0; g < RW / 4; ++g) {
            if (row0 + 4 * g >= N) break;                  // (uniform over the wave)
            RbRow row[4];                                  // a row past the pool's end is the last row again, its result dropped
            float4 x0[4], x1[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const long long n = row0 + 4 * g + a;
                row[a] = rb_row<PAIR>(t, n < N ? n : N - 1);
                x0[a] = x1[a] = zero;
                if constexpr (SHORT) {
                    if (4 * lane < D) x0[a] = rb_quad<PAIR, VEC>(row[a], 4 * lane, D);
                    if (4 * lane + 256 < D) x1[a] = rb_quad<PAIR, VEC>(row[a], 4 * lane + 256, D);
                }
            }
            for (int m = 0; m < tm; m += 4) {
                const float* z[4];                         // a row past the tile's last is that last row again: no minimum changes
                float s[16];
#pragma unroll
                for (int b = 0; b < 4; ++b) z[b] = tile + (m + b < tm ? m + b : tm - 1) * Dp + 4 * lane;
#pragma unroll
                for (int j = 0; j < 16; ++j) s[j] = 0.f;
                if constexpr (SHORT) {
                    if (4 * lane < D) {
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const float4 p = *(const float4*)z[b];
#pragma unroll
                            for (int a = 0; a < 4; ++a) s[4 * a + b] = rb_acc(s[4 * a + b], x0[a], p);
                        }
                    }
                    if (4 * lane + 256 < D) {
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const float4 p = *(const float4*)(z[b] + 256);
#pragma unroll
                            for (int a = 0; a < 4; ++a) s[4 * a + b] = rb_acc(s[4 * a + b], x1[a], p);
                        }
                    }
                } else {
                    for (int e = 0; 4 * lane + e < D; e += 256) {
#pragma unroll
                        for (int a = 0; a < 4; ++a) x0[a] = rb_quad<PAIR, VEC>(row[a], 4 * lane + e, D);
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const float4 p = *(const float4*)(z[b] + e);
#pragma unroll
                            for (int a = 0; a < 4; ++a) s[4 * a + b] = rb_acc(s[4 * a + b], x0[a], p);
                        }
                    }
                }
                const float v = rb_block_row_minima(s, lane);
                if ((lane & 15) == g) best = fminf(best, v);
            }
        }
    }
    const int q = 4 * (lane & 15) + (lane >> 4);
    if ((lane & 15) < RW / 4 && row0 + q < N) d2[row0 + q] = best;
}

// the workgroup's 256 threads reduce `nparts` partials; every thread returns the winner
__device__ __forceinline__ RbCand rb_reduce_partials(const RbCand* __restrict__ parts, int nparts, RbCand* s_w) {
    RbCand c{-INFINITY, RB_NONE};
    for (int i = threadIdx.x; i < nparts; i += 256) c = rb_better(c, parts[i]);
    c = rb_wave_max(c);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    c = s_w[0];
    for (int w = 1; w < 4; ++w) c = rb_better(c, s_w[w]);
    return c;
}

template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256) void rb_step_kernel(const RbRows t, long long N, float* __restrict__ d2, const float* __restrict__ util,
                                                      float alpha, int step, const RbCand* __restrict__ prev_parts,
                                                      RbCand* __restrict__ out_parts, int32_t* __restrict__ idx_out,
                                                      float* __restrict__ score_out) {
    extern __shared__ float4 rb_dynamic_lds[];             // the picked row: D rounded up to a multiple of 4 floats
    float* prow = (float*)rb_dynamic_lds;
    __shared__ RbCand s_prev[4], s_best[4];
    constexpr int NR = RB_PASS_ROWS;
    const int D = t.D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long pick = -1;                                   // the previous launch's pick: -1 in the first launch, or when
    if (step > 0) {                                        // nothing but NaN scores was left
        const RbCand c = rb_reduce_partials(prev_parts, (int)gridDim.x, s_prev);
        if (c.i != RB_NONE) pick = c.i;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            idx_out[step - 1] = c.i != RB_NONE ? c.i : -1;
            score_out[step - 1] = c.v;
        }
        if (pick >= 0) rb_stage_row<PAIR>(rb_row<PAIR>(t, pick), D, (D + 3) & ~3, prow);
        __syncthreads();
    }
    const float one_minus_alpha = 1.f - alpha;
    RbCand best{-INFINITY, RB_NONE};
    const long long stride = (long long)gridDim.x * 4 * NR;
    for (long long n0 = ((long long)blockIdx.x * 4 + wave) * NR; n0 < N; n0 += stride) {
        long long n[NR];
        float d[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            n[j] = n0 + j < N ? n0 + j : n0;               // past the pool's end: row n0 again, that result dropped
            d[j] = d2[n[j]];
        }
        if (pick >= 0) {
            RbRow r[NR];
            float s[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                r[j] = rb_row<PAIR>(t, n[j]);
                s[j] = 0.f;
            }
            for (int e0 = 4 * lane; e0 < D; e0 += 256) {
                const float4 p = *(const float4*)(prow + e0);
#pragma unroll
                for (int j = 0; j < NR; ++j) s[j] = rb_acc(s[j], rb_quad<PAIR, VEC>(r[j], e0, D), p);
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const float sj = rb_wave_sum(s[j]);
                if (!(d[j] < 0.f)) d[j] = n[j] == pick ? -1.f : fminf(d[j], sj);
                if (lane == 0 && n0 + j < N) d2[n[j]] = d[j];
            }
        }
#pragma unroll
        for (int j = 0; j < NR; ++j)
            if (n0 + j < N && !(d[j] < 0.f)) best = rb_better(best, RbCand{rb_score(d[j], util[n[j]], alpha, one_minus_alpha), (int)n[j]});
    }
    if (lane == 0) s_best[wave] = best;                    // (every lane of a wave holds the same candidate)
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = rb_better(best, s_best[w]);
        out_parts[blockIdx.x] = best;
    }
}

__global__ __launch_bounds__(256) void rb_finish_kernel(const RbCand* __restrict__ parts, int nparts, int last, int32_t* __restrict__ idx_out,
                                                        float* __restrict__ score_out) {
    __shared__ RbCand s_w[4];
    const RbCand c = rb_reduce_partials(parts, nparts, s_w);
    if (threadIdx.x == 0) {
        idx_out[last] = c.i != RB_NONE ? c.i : -1;
        score_out[last] = c.v;
    }
}

size_t rb_d2_bytes(int64_t N) { return ((size_t)N * 4 + 255) & ~(size_t)255; }

template <bool PAIR, bool VEC>
void rb_enqueue(const RbRows& t, long long N, const float* labeled, long long M, const float* util, int k, float alpha, int32_t* idx,
                float* scores, float* d2, RbCand* parts, hipStream_t st) {
    const int Dp = (t.D + 3) & ~3;
    const int tile_rows = RB_MAX_D / Dp;                   // >= 1: D <= RB_MAX_D; >= 16 for D <= 512
    const unsigned init_blocks = (unsigned)((N + RB_WG_ROWS - 1) / RB_WG_ROWS);
    if (t.D <= 512) hipLaunchKernelGGL((rb_init_kernel<PAIR, VEC, true>), dim3(init_blocks), dim3(256), 0, st, t, N, labeled, M, tile_rows, d2);
    else hipLaunchKernelGGL((rb_init_kernel<PAIR, VEC, false>), dim3(init_blocks), dim3(256), 0, st, t, N, labeled, M, tile_rows, d2);
    const long long want = (N + 4 * RB_PASS_ROWS - 1) / (4 * RB_PASS_ROWS);
    const unsigned grid = (unsigned)(want < RB_MAX_GRID ? want : RB_MAX_GRID);
    for (int s = 0; s < k; ++s) {
        // picks count as labelled: |unlabelled| / (|unlabelled| + |labelled|) = (N - s) / (N + M), the float32 of the float64 quotient
        const float a = alpha < 0.f ? (float)((double)(N - s) / (double)(N + M)) : alpha;
        hipLaunchKernelGGL((rb_step_kernel<PAIR, VEC>), dim3(grid), dim3(256), (size_t)Dp * 4, st, t, N, d2, util, a, s,
                           parts + (size_t)((s + 1) & 1) * RB_MAX_GRID, parts + (size_t)(s & 1) * RB_MAX_GRID, idx, scores);
    }
    hipLaunchKernelGGL(rb_finish_kernel, dim3(1), dim3(256), 0, st, parts + (size_t)((k - 1) & 1) * RB_MAX_GRID, (int)grid, k - 1, idx, scores);
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

size_t alink_ranked_batch_scratch_bytes(int64_t N, int k) {
    if (N <= 0 || k <= 0) return 0;
    return rb_d2_bytes(N) + 2 * (size_t)RB_MAX_GRID * sizeof(RbCand);
}

int alink_ranked_batch(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                       const float* dev_labeled, int64_t M, const float* dev_utility, int k, float alpha, int32_t* dev_idx,
                       float* dev_scores, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_x && dev_utility && dev_idx && dev_scores && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_li || (dev_r && dev_ri), ALINK_EINVAL, "the pair form needs dev_r and dev_ri beside dev_li");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d (the picked row is held in LDS)", D, RB_MAX_D);
    ALINK_REQUIRE(M >= 1, ALINK_EINVAL, "M=%lld: ranked batch selection on the device needs at least one labelled row (the cold "
                  "start, the row nearest to all others, is O(N^2 D) and stays on the host)", (long long)M);
    ALINK_REQUIRE(dev_labeled, ALINK_EINVAL, "NULL labelled rows");
    ALINK_REQUIRE(k >= 1, ALINK_EINVAL, "k=%d must be >= 1", k);
    ALINK_REQUIRE(!(alpha > 1.f) && alpha == alpha, ALINK_EINVAL, "alpha=%g: a weight in [0, 1], or negative for the schedule", (double)alpha);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    if ((int64_t)k > N) k = (int)N;
    DeviceGuard dg(device_of_pointer(dev_x));
    RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    float* d2 = (float*)dev_scratch;
    RbCand* parts = (RbCand*)((char*)dev_scratch + rb_d2_bytes(N));
    hipStream_t st = (hipStream_t)stream;
    const bool pair = dev_li != nullptr;
    const bool vec = D % 4 == 0 && (((uintptr_t)dev_x | (pair ? (uintptr_t)dev_r : 0)) & 15) == 0;
    if (pair) {
        if (vec) rb_enqueue<true, true>(t, N, dev_labeled, M, dev_utility, k, alpha, dev_idx, dev_scores, d2, parts, st);
        else rb_enqueue<true, false>(t, N, dev_labeled, M, dev_utility, k, alpha, dev_idx, dev_scores, d2, parts, st);
    } else {
        if (vec) rb_enqueue<false, true>(t, N, dev_labeled, M, dev_utility, k, alpha, dev_idx, dev_scores, d2, parts, st);
        else rb_enqueue<false, false>(t, N, dev_labeled, M, dev_utility, k, alpha, dev_idx, dev_scores, d2, parts, st);
    }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
