// knn.hip — the K nearest neighbours of every pool row among the pool's other rows, their distances and the typicality of
// TypiClust (Hacohen, Dekel & Weinshall 2022: the inverse of the mean distance to the K nearest neighbours), and the per-group
// argmax that turns typicalities into queries (a-link_amd/typiclust.py).  include/alink_hip.h (alink_knn, alink_group_argmax)
// states the rule in full.
//
// What bounds it: an (N x D)(D x N) product on the f32 matrix cores whose scores never reach memory — the tile product of
// pool_tile.h (which describes the geometry and why x_n . x_j is ONE ascending fmaf chain whatever tile either row falls in) with
// the pool as its own candidates, and a running sorted list of K where kmeans.hip keeps a running minimum.
//
// Launches of alink_knn, all on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative launch,
// no grid barrier, no atomics, nothing read back):
//   pt_norm_kernel  (pool_tile.h) |x_j|^2 of every row, one wave per row, in the summation order of batch_rows.h
//   kn_list_kernel  pt_product per tile of 128 candidates, the tile's norms and groups staged beside the operands.  In a lane the
//                   16 candidates of a block come in ascending order, so a strict `<` keeps the lower candidate among ties.  The
//                   lane's running KK best are a sorted list of (score, index) in registers (KK = 8 / 16 / 32 at compile time,
//                   every index a constant: a smaller K is the head of the next larger list); a candidate enters through an
//                   unrolled compare-and-shift chain, which only those candidates walk that SOME lane of the wave holds below its
//                   KK-th — a wave-uniform vote per candidate, gathered into a 16-bit mask per MFMA block and worked off in
//                   ascending order, so the chain stands four times in the code, not 64.  At the end the two lanes of a row
//                   exchange their lists with lane ^ 32 and merge them on (score, index): min(A[i], B[KK - 1 - i]) is a bitonic
//                   sequence of the KK least, log2(KK) half-cleaner stages sort it.
//   kn_dist_kernel  the light pass, one wave per row: d2 of the K winners by direct differences in batch_rows.h's order, and the
//                   float64 mean of the typicality in ascending slot order.
// alink_group_argmax is two launches in the shape of km_accum_kernel / km_final_kernel: wave (g, s) scans slice s of the group
// vector in ascending row order, then one thread per group combines the slices in ascending order.
// Measured: DESIGN.md §9.  Not built: skipping candidate tiles that hold no row of the workgroup's groups, K > 32, a cosine
// metric, several ranks' pools in one call.  (Queries against a separate reference set: knn_rect.hip, which shares the list
// helpers of knn_lists.h with this file.)
#include "knn_lists.h"

namespace alink {
namespace {

constexpr int KN_MAX_G = 8192;

// Two waves per SIMD, as the assignment kernel has: asked for, because left alone the compiler spends 255 + 80 registers at
// KK = 32 and fits one.  The one form that does not fit 256 registers without scratch — KK = 32 on a row table read with scalar
// loads — keeps one wave.
template <int KK, bool PAIR, bool VEC>
__global__ __launch_bounds__(256, (KK == 32 && !PAIR && !VEC) ? 1 : 2) void kn_list_kernel(const RbRows t, long long N, const float* __restrict__ xnorm,
                                                      const int32_t* __restrict__ group, int K, int32_t* __restrict__ idx,
                                                      int32_t* __restrict__ found) {
    __shared__ float sX[PT_DC * PT_LD];
    __shared__ float sC[PT_DC * PT_LD];
    __shared__ __attribute__((aligned(16))) float sN[PT_TK];
    __shared__ __attribute__((aligned(16))) int sG[PT_TK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const long long n0 = (long long)blockIdx.x * PT_TN;
    const int srow = tid & 127;            // the tile row this thread stages (pool_tile.h)
    const long long xn = n0 + srow;
    const bool xhave = xn < N;

    // this lane's row: its index, and its group — -2, which no candidate carries (no neighbours), past the pool, in a group < 0, or
    // with |x|^2 NaN or +inf
    const long long n = n0 + wave * 32 + l31;
    int gn = -2;
    if (n < N) {
        gn = group ? group[n] : 0;
        if (gn < 0 || !(xnorm[n] < INFINITY)) gn = -2;
    }
    const int self = n < N ? (int)n : -1;

    float ls[KK];                          // a score enters by `<` alone: neither NaN nor +inf ever does
    int lj[KK];
#pragma unroll
    for (int p = 0; p < KK; ++p) { ls[p] = INFINITY; lj[p] = -1; }

    for (long long k0 = 0; k0 < N; k0 += PT_TK) {
        const long long left = N - k0;
        const int nblk = left >= PT_TK ? 4 : (int)((left + 31) >> 5);      // MFMA row blocks of this tile that hold a row (uniform)
        const long long cn_ = k0 + srow;
        const bool chave = cn_ < N;
        f32x16 acc[4];
        pt_product<PAIR, VEC, PAIR, VEC>(t, xn, xhave, t, cn_, chave, nblk, sX, sC, acc, [&](int i) {
            const long long j = k0 + i;
            sN[i] = j < N ? xnorm[j] : INFINITY;           // a padded candidate never enters
            const int gj = j < N ? (group ? group[j] : 0) : -1;
            sG[i] = gj < 0 ? -1 : gj;                      // every group < 0 is -1 here: nobody's neighbour
        });
        // the tile's scores against the running list: in a lane the candidates come in ascending order
        const int jbase = (int)(unsigned)k0 + 4 * hh;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nblk) {
                // the block's 16 scores of this lane, and which of them SOME lane of the wave holds below its KK-th (uniform): only
                // those walk the insertion chain, in ascending order.  (A list's KK-th only falls, so a candidate that is not
                // marked against the KK-th of before the block's insertions would not have entered after them either, and a
                // marked one that no longer enters leaves the list as it is.)
                float sc[16];
                unsigned marked = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 cn = *(const float4*)(sN + b * 32 + 8 * g + 4 * hh);
                    const int4 cg = *(const int4*)(sG + b * 32 + 8 * g + 4 * hh);
                    const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
                    const int cgv[4] = {cg.x, cg.y, cg.z, cg.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = jbase + b * 32 + 8 * g + i;
                        const float s = __builtin_fmaf(-2.f, acc[b][4 * g + i], cnv[i]);
                        sc[4 * g + i] = (cgv[i] == gn && j != self) ? s : INFINITY;
                        marked |= __ballot(sc[4 * g + i] < ls[KK - 1]) != 0ull ? 1u << (4 * g + i) : 0u;
                    }
                }
#pragma unroll 1
                while (marked) {
                    const int r = __ffs(marked) - 1;
                    marked &= marked - 1;
                    kn_insert<KK>(ls, lj, kn_pick16(sc, r), jbase + b * 32 + 8 * (r >> 2) + (r & 3));
                }
            }
        }
    }
    kn_merge_halves<KK>(ls, lj);           // the two halves of a row meet
    if (hh == 0 && n < N) {
        int32_t* o = idx + (size_t)n * K;
        int f = 0;
#pragma unroll
        for (int p = 0; p < KK; ++p)
            if (p < K) { o[p] = lj[p]; f += lj[p] >= 0; }
        if (found) found[n] = f;
    }
}

// the light pass, one wave per row: d2 of the winners, the typicality
template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256) void kn_dist_kernel(const RbRows t, long long N, int K, const int32_t* __restrict__ idx, int squared,
                                                      double eps, float* __restrict__ d2, float* __restrict__ typicality) {
    const int D = t.D;
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const RbRow r = rb_row<PAIR>(t, n);
    double sum = 0.0;                                      // the found slots in ascending order (every lane holds the same)
    int f = 0;
    for (int p = 0; p < K; ++p) {
        const int j = idx[(size_t)n * K + p];
        float d = __builtin_nanf("");
        if (j >= 0) {                                      // (uniform over the wave)
            const RbRow c = rb_row<PAIR>(t, j);
            float s = 0.f;
            for (int e0 = 4 * lane; e0 < D; e0 += 256) s = rb_acc(s, rb_quad<PAIR, VEC>(r, e0, D), rb_quad<PAIR, VEC>(c, e0, D));
            d = rb_wave_sum(s);
            sum += squared ? (double)d : sqrt((double)d);
            ++f;
        }
        if (lane == 0 && d2) d2[(size_t)n * K + p] = d;
    }
    if (lane == 0 && typicality) typicality[n] = f ? (float)(1.0 / (sum / (double)f + eps)) : 0.f;
}

// wave (g, s): the rows of group g in slice s, ascending; the largest value by `>` from -inf, ties to the lower row
__global__ __launch_bounds__(64) void ga_scan_kernel(const float* __restrict__ value, const int32_t* __restrict__ group, long long N,
                                                     long long slice, int S, float* __restrict__ pval, int32_t* __restrict__ prow) {
    const int lane = threadIdx.x, g = blockIdx.x, s = blockIdx.y;
    const long long r0 = (long long)s * slice, r1 = r0 + slice < N ? r0 + slice : N;
    float bv = -INFINITY;
    int br = -1;
    for (long long base = r0; base < r1; base += 64) {
        const long long n = base + lane;
        if (n < r1 && group[n] == g) {
            const float v = value[n];
            if (v > bv) { bv = v; br = (int)n; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int orow = __shfl_xor(br, o, 64);
        if (orow >= 0 && (br < 0 || ov > bv || (ov == bv && orow < br))) { bv = ov; br = orow; }
    }
    if (lane == 0) { pval[(size_t)g * S + s] = bv; prow[(size_t)g * S + s] = br; }
}

// one thread per group: the slices' winners in ascending order
__global__ __launch_bounds__(256) void ga_final_kernel(int G, int S, const float* __restrict__ pval, const int32_t* __restrict__ prow,
                                                       int32_t* __restrict__ best) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    float bv = -INFINITY;
    int br = -1;
    for (int s = 0; s < S; ++s) {
        const float v = pval[(size_t)g * S + s];
        const int r = prow[(size_t)g * S + s];
        if (r >= 0 && v > bv) { bv = v; br = r; }
    }
    best[g] = br;
}

struct KnArgs {
    const int32_t* group;
    int K, squared;
    double eps;
    int32_t* idx;
    float* d2;
    int32_t* found;
    float* typicality;
};

template <bool PAIR, bool VEC>
void kn_enqueue(const RbRows& t, long long N, const KnArgs& a, float* xnorm, hipStream_t st) {
    const unsigned wgrid = (unsigned)((N + 3) / 4);
    const unsigned lgrid = (unsigned)((N + PT_TN - 1) / PT_TN);
    hipLaunchKernelGGL((pt_norm_kernel<PAIR, VEC>), dim3(wgrid), dim3(256), 0, st, t, N, xnorm);
    if (a.K <= 8)
        hipLaunchKernelGGL((kn_list_kernel<8, PAIR, VEC>), dim3(lgrid), dim3(256), 0, st, t, N, xnorm, a.group, a.K, a.idx, a.found);
    else if (a.K <= 16)
        hipLaunchKernelGGL((kn_list_kernel<16, PAIR, VEC>), dim3(lgrid), dim3(256), 0, st, t, N, xnorm, a.group, a.K, a.idx, a.found);
    else
        hipLaunchKernelGGL((kn_list_kernel<32, PAIR, VEC>), dim3(lgrid), dim3(256), 0, st, t, N, xnorm, a.group, a.K, a.idx, a.found);
    if (a.d2 || a.typicality)
        hipLaunchKernelGGL((kn_dist_kernel<PAIR, VEC>), dim3(wgrid), dim3(256), 0, st, t, N, a.K, a.idx, a.squared, a.eps, a.d2,
                           a.typicality);
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

size_t alink_knn_scratch_bytes(int64_t N, int D, int K) {
    if (N <= 0 || N >= (1ll << 31) || D <= 0 || D > RB_MAX_D || K <= 0 || K > KN_MAX_K) return 0;
    return pt_align((size_t)N * 4);
}

int alink_knn(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
              const int32_t* dev_group, int K, int squared, double eps, int32_t* dev_idx, float* dev_d2, int32_t* dev_found,
              float* dev_typicality, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_x && dev_idx && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_li || (dev_r && dev_ri), ALINK_EINVAL, "the pair form needs dev_r and dev_ri beside dev_li");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d", D, RB_MAX_D);
    ALINK_REQUIRE(K >= 1 && K <= KN_MAX_K, ALINK_EINVAL, "K=%d outside 1..%d", K, KN_MAX_K);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_x));
    RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    const KnArgs a{dev_group, K, squared ? 1 : 0, eps, dev_idx, dev_d2, dev_found, dev_typicality};
    hipStream_t st = (hipStream_t)stream;
    const bool pair = dev_li != nullptr;
    const bool vec = pt_vec(t);
    float* xnorm = (float*)dev_scratch;
    if (pair) { if (vec) kn_enqueue<true, true>(t, N, a, xnorm, st); else kn_enqueue<true, false>(t, N, a, xnorm, st); }
    else { if (vec) kn_enqueue<false, true>(t, N, a, xnorm, st); else kn_enqueue<false, false>(t, N, a, xnorm, st); }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

size_t alink_group_argmax_scratch_bytes(int64_t N, int G) {
    if (N <= 0 || N >= (1ll << 31) || G <= 0 || G > KN_MAX_G) return 0;
    long long slice;
    const size_t S = (size_t)pt_slices(N, G, &slice);
    return pt_align((size_t)G * S * 4) * 2;
}

int alink_group_argmax(const float* dev_value, const int32_t* dev_group, int64_t N, int G, int32_t* dev_best, void* dev_scratch,
                       void* stream) {
    ALINK_REQUIRE(dev_value && dev_group && dev_best && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(G >= 1 && G <= KN_MAX_G, ALINK_EINVAL, "G=%d outside 1..%d", G, KN_MAX_G);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_value));
    long long slice;
    const int S = pt_slices(N, G, &slice);
    float* pval = (float*)dev_scratch;
    int32_t* prow = (int32_t*)((char*)dev_scratch + pt_align((size_t)G * S * 4));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ga_scan_kernel, dim3(G, S), dim3(64), 0, st, dev_value, dev_group, (long long)N, slice, S, pval, prow);
    hipLaunchKernelGGL(ga_final_kernel, dim3((G + 255) / 256), dim3(256), 0, st, G, S, pval, prow, dev_best);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
