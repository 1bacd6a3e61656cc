// probcover.hip — the fixed-radius neighbour graph of a pool (every row's ball of radius delta, as CSR), the nearest row of another
// group that gives the purity curve, and the greedy maximum coverage over that graph: ProbCover (Yehuda, Dekel, Hacohen &
// Weinshall 2022, "Active Learning Through a Covering Lens"; a-link_amd/probcover.py).  include/alink_hip.h (alink_ball_count,
// alink_ball_fill, alink_max_coverage) states the rule in full.
//
// What bounds the graph: the (N x D)(D x N) product of knn.hip on the f32 matrix cores — the tile product of pool_tile.h — whose
// scores never reach memory, with a threshold in place of the running lists.  x_n . x_j is ONE ascending fmaf chain whatever tile
// either row falls in (pool_tile.h), the same bits for (n, j) and (j, n); the two norms meet in one float32 addition, which
// commutes: t(n, j) and t(j, n) are the same bits and the graph is symmetric.
//
// Launches, all on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative launch, no grid
// barrier, no atomics, nothing read back):
//   pt_norm_kernel   (pool_tile.h) |x_j|^2 of every row, one wave per row, in the summation order of batch_rows.h
//   pb_tile_kernel   pt_product per tile of 128 candidates, the tile's norms and groups (-1: not eligible) staged beside the
//                    operands.  Lane (l, h) of a wave holds for row l the 16 candidates 8 g + 4 h + i of each block.  pb_block —
//                    the ONE place the score is formed and the edge decided — gives the lane's 16 decisions as bits at their
//                    candidate positions of a 32-bit mask.
//                    Counting form: popc of the mask, and (with groups) the running minimum over rows of another group; the two
//                    lanes of a row (lane ^ 32) add their counts and combine their minima on (t, j) at the end.
//                    Filling form: the two lanes OR their masks, a lane writes its candidate c at offsets[n] + base + popc(mask
//                    below c), base += popc(mask): ascending order, every slot written once, no atomics.  A write outside
//                    [offsets[n], offsets[n + 1]) or [0, E) is dropped, and a row whose ball did not exactly fill its span is
//                    flagged; pb_flag_sum_kernel (one workgroup) adds the flags into dev_mismatch.
//   mc_seed_kernel   one wave per seed row: its ball covered
//   mc_count_kernel  per pick: workgroup = a contiguous chunk of 64 rows, 16 per wave; a wave strides a row's span of nbr and counts
//                    the rows not yet covered; the chunk's (largest degree, lowest row) goes to scratch
//   mc_pick_kernel   per pick: ONE workgroup combines the chunks in ascending order, writes pick and gain, marks ball(pick) with
//                    plain byte stores of 1
// Measured: DESIGN.md §9.  Not built: distances stored with the edges, skipping tiles by a spatial bound, an incremental-degree
// greedy, a cosine metric, balls round a separate set of centres (knn_rect.hip has the rectangular product, for lists of K, not
// for balls), several ranks' pools in one call.
#include "pool_tile.h"

namespace alink {
namespace {

constexpr int MC_ROWS = 64;                // rows of a chunk of the recount: 16 per wave

enum { PB_DEGREE = 0, PB_OTHER = 1, PB_FILL = 2 };

// The score and the edge test, the same code in the counting and the filling pass.  One float32 addition (it commutes), one
// fused rounding: t(n, j) and t(j, n) are the same bits.
__device__ __forceinline__ float pb_score(float dot, float xn_n, float xn_j) { return __builtin_fmaf(-2.f, dot, xn_n + xn_j); }
// gn, gj: the group of an eligible row, < 0 otherwise
__device__ __forceinline__ bool pb_edge(float t, float radius2, int gn, int gj, bool self) {
    return gn >= 0 && gj >= 0 && (self || t < radius2);
}

// One MFMA block against this lane's row: the lane's 16 decisions as bits 8 g + 4 h + i of the block's 32 candidates.  j0 = the
// index of the block's candidate 4 h; sNb, sGb = the block's norms and groups in LDS.  PB_OTHER: (tb, jb) = the running least t
// over eligible candidates of another group, by `<` (a lane's candidates come in ascending order: ties keep the lower j).
template <int MODE>
__device__ __forceinline__ unsigned pb_block(const f32x16& acc, const float* sNb, const int* sGb, int hh, float xnn, int gn, int self,
                                             int j0, float radius2, float& tb, int& jb) {
    unsigned m = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 cn = *(const float4*)(sNb + 8 * g + 4 * hh);
        const int4 cg = *(const int4*)(sGb + 8 * g + 4 * hh);
        const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
        const int cgv[4] = {cg.x, cg.y, cg.z, cg.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = j0 + 8 * g + i;
            const float t = pb_score(acc[4 * g + i], xnn, cnv[i]);
            m |= pb_edge(t, radius2, gn, cgv[i], j == self) ? 1u << (8 * g + i) : 0u;
            if constexpr (MODE == PB_OTHER) {
                const bool less = gn >= 0 && cgv[i] >= 0 && cgv[i] != gn && t < tb;
                tb = less ? t : tb;
                jb = less ? j : jb;
            }
        }
    }
    return m << (4 * hh);
}

struct PbOut {
    float radius2;
    int32_t* deg;                          // counting forms (each may be NULL)
    float* t_other;
    int32_t* j_other;
    const long long* offsets;              // filling form
    long long E;
    int32_t* nbr;
    int32_t* flag;                         // (N) 1 = the row's ball did not exactly fill its span
};

// Two waves per SIMD, as kn_list_kernel has.
template <int MODE, bool PAIR, bool VEC>
__global__ __launch_bounds__(256, 2) void pb_tile_kernel(const RbRows t, long long N, const float* __restrict__ xnorm,
                                                          const int32_t* __restrict__ group, const PbOut o) {
    __shared__ float sX[PT_DC * PT_LD];
    __shared__ float sC[PT_DC * PT_LD];
    __shared__ __attribute__((aligned(16))) float sN[PT_TK];
    __shared__ __attribute__((aligned(16))) int sG[PT_TK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const long long n0 = (long long)blockIdx.x * PT_TN;
    const int srow = tid & 127;            // the tile row this thread stages (pool_tile.h)
    const long long xn = n0 + srow;
    const bool xhave = xn < N;

    // this lane's row: its index, its norm and its group — -2 (no ball, in nobody's ball) past the pool, in a group < 0, or with
    // |x|^2 NaN or +inf
    const long long n = n0 + wave * 32 + l31;
    int gn = -2;
    float xnn = 0.f;
    if (n < N) {
        xnn = xnorm[n];
        gn = group ? group[n] : 0;
        if (gn < 0 || !(xnn < INFINITY)) gn = -2;
    }
    const int self = n < N ? (int)n : -1;
    const float radius2 = o.radius2;

    int cnt = 0;                           // PB_DEGREE, PB_OTHER: this lane's share of the degree; PB_FILL: the row's edges so far
    float tb = INFINITY;
    int jb = -1;
    long long o0 = 0, o1 = 0;
    if constexpr (MODE == PB_FILL) {
        if (n < N) { o0 = o.offsets[n]; o1 = o.offsets[n + 1]; }
    }

    for (long long k0 = 0; k0 < N; k0 += PT_TK) {
        const long long left = N - k0;
        const int nblk = left >= PT_TK ? 4 : (int)((left + 31) >> 5);      // MFMA row blocks of this tile that hold a row (uniform)
        const long long cn_ = k0 + srow;
        const bool chave = cn_ < N;
        f32x16 acc[4];
        pt_product<PAIR, VEC, PAIR, VEC>(t, xn, xhave, t, cn_, chave, nblk, sX, sC, acc, [&](int i) {
            const long long j = k0 + i;
            const float nj = j < N ? xnorm[j] : INFINITY;
            const int gj = j < N ? (group ? group[j] : 0) : -1;
            sN[i] = nj;
            sG[i] = (gj < 0 || !(nj < INFINITY)) ? -1 : gj;                // -1: not eligible (or past the pool) — in nobody's ball
        });
        const int jbase = (int)(unsigned)k0 + 4 * hh;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nblk) {
                const unsigned mine = pb_block<MODE>(acc[b], sN + b * 32, sG + b * 32, hh, xnn, gn, self, jbase + b * 32, radius2, tb, jb);
                if constexpr (MODE != PB_FILL) {
                    cnt += __popc(mine);
                } else {
                    const unsigned both = mine | (unsigned)__shfl_xor((int)mine, 32, 64);
                    if (mine) {
#pragma unroll
                        for (int g = 0; g < 4; ++g)
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int c = 8 * g + i + 4 * hh;
                                const long long pos = o0 + cnt + __popc(both & ((1u << c) - 1u));
                                if (((mine >> c) & 1u) && pos >= 0 && pos < o1 && pos < o.E) o.nbr[pos] = jbase + b * 32 + 8 * g + i;
                            }
                    }
                    cnt += __popc(both);
                }
            }
        }
    }
    if constexpr (MODE == PB_FILL) {
        if (hh == 0 && n < N) o.flag[n] = (o0 < 0 || o1 > o.E || (long long)cnt != o1 - o0) ? 1 : 0;
    } else {
        cnt += __shfl_xor(cnt, 32, 64);    // the two halves of a row meet
        if constexpr (MODE == PB_OTHER) {
            const float ot = __shfl_xor(tb, 32, 64);
            const int oj = __shfl_xor(jb, 32, 64);
            const bool take = oj >= 0 && (jb < 0 || ot < tb || (ot == tb && oj < jb));
            tb = take ? ot : tb;
            jb = take ? oj : jb;
        }
        if (hh == 0 && n < N) {
            if (o.deg) o.deg[n] = cnt;
            if constexpr (MODE == PB_OTHER) {
                if (o.t_other) o.t_other[n] = tb;
                if (o.j_other) o.j_other[n] = jb;
            }
        }
    }
}

// the flagged rows, added by one workgroup (integers: the order is immaterial) and stored once
__global__ __launch_bounds__(256) void pb_flag_sum_kernel(const int32_t* __restrict__ flag, long long N, int32_t* __restrict__ out) {
    __shared__ int part[256];
    int s = 0;
    for (long long n = threadIdx.x; n < N; n += 256) s += flag[n];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

template <int MODE, bool PAIR, bool VEC>
void pb_enqueue(const RbRows& t, long long N, const int32_t* group, const PbOut& o, float* xnorm, hipStream_t st) {
    hipLaunchKernelGGL((pt_norm_kernel<PAIR, VEC>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, t, N, xnorm);
    hipLaunchKernelGGL((pb_tile_kernel<MODE, PAIR, VEC>), dim3((unsigned)((N + PT_TN - 1) / PT_TN)), dim3(256), 0, st, t, N, xnorm, group, o);
    if (MODE == PB_FILL) hipLaunchKernelGGL(pb_flag_sum_kernel, dim3(1), dim3(256), 0, st, o.flag, N, (int32_t*)o.deg);
}

template <int MODE>
void pb_dispatch(const RbRows& t, long long N, const int32_t* group, const PbOut& o, float* xnorm, hipStream_t st) {
    const bool pair = t.li != nullptr;
    const bool vec = pt_vec(t);
    if (pair) { if (vec) pb_enqueue<MODE, true, true>(t, N, group, o, xnorm, st); else pb_enqueue<MODE, true, false>(t, N, group, o, xnorm, st); }
    else { if (vec) pb_enqueue<MODE, false, true>(t, N, group, o, xnorm, st); else pb_enqueue<MODE, false, false>(t, N, group, o, xnorm, st); }
}

// ---- greedy maximum coverage -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mc_wave_sum(int s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// one wave per seed: every row of its ball is covered.  A seed outside 0 .. N - 1 is ignored.
__global__ __launch_bounds__(256) void mc_seed_kernel(const long long* __restrict__ offsets, const int32_t* __restrict__ nbr, long long N,
                                                      const int32_t* __restrict__ seed, long long S, uint8_t* __restrict__ covered) {
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;
    const long long u = seed[s];
    if (u < 0 || u >= N) return;
    const long long o1 = offsets[u + 1];
    for (long long e = offsets[u] + lane; e < o1; e += 64) {
        const unsigned v = (unsigned)nbr[e];
        if ((long long)v < N) covered[v] = 1;
    }
}

// the recount: chunk = MC_ROWS contiguous rows, a quarter per wave in ascending order; a wave strides the row's span of nbr
__global__ __launch_bounds__(256) void mc_count_kernel(const long long* __restrict__ offsets, const int32_t* __restrict__ nbr, long long N,
                                                       const uint8_t* __restrict__ covered, int32_t* __restrict__ cdeg,
                                                       int32_t* __restrict__ crow) {
    __shared__ int sdeg[4], srow[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * MC_ROWS + wave * (MC_ROWS / 4);
    int best = 0, brow = -1;
    for (int i = 0; i < MC_ROWS / 4; ++i) {
        const long long u = r0 + i;
        if (u >= N) break;                                 // (uniform over the wave)
        const long long o0 = offsets[u], o1 = offsets[u + 1];
        if (o0 >= o1) continue;
        int c = 0;
        for (long long e = o0 + lane; e < o1; e += 64) {
            const unsigned v = (unsigned)nbr[e];
            c += ((long long)v < N && covered[v] == 0) ? 1 : 0;
        }
        c = mc_wave_sum(c);
        if (c > best) { best = c; brow = (int)u; }         // `>`: among equal degrees the lower row stays
    }
    if (lane == 0) { sdeg[wave] = best; srow[wave] = brow; }
    __syncthreads();
    if (threadIdx.x == 0) {
        best = 0; brow = -1;
        for (int w = 0; w < 4; ++w)
            if (sdeg[w] > best) { best = sdeg[w]; brow = srow[w]; }
        cdeg[blockIdx.x] = best;
        crow[blockIdx.x] = brow;
    }
}

// ONE workgroup: the chunks' (largest degree, lowest row) in ascending order, the pick, its gain, its ball covered
__global__ __launch_bounds__(256) void mc_pick_kernel(const long long* __restrict__ offsets, const int32_t* __restrict__ nbr, long long N,
                                                      const int32_t* __restrict__ cdeg, const int32_t* __restrict__ crow, long long C,
                                                      int t, int32_t* __restrict__ picks, int32_t* __restrict__ gain,
                                                      uint8_t* __restrict__ covered) {
    __shared__ int sdeg[256], srow[256];
    const int tid = threadIdx.x;
    int best = 0, brow = -1;
    for (long long c = tid; c < C; c += 256) {             // a thread's chunks ascend: `>` keeps the lower row
        const int d = cdeg[c];
        if (d > best) { best = d; brow = crow[c]; }
    }
    sdeg[tid] = best; srow[tid] = brow;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {                                     // (degree descending, row ascending): the same winner in any order
            const int d = sdeg[tid + w], r = srow[tid + w];
            if (d > sdeg[tid] || (d == sdeg[tid] && d > 0 && r < srow[tid])) { sdeg[tid] = d; srow[tid] = r; }
        }
        __syncthreads();
    }
    best = sdeg[0]; brow = srow[0];
    if (tid == 0) { picks[t] = best > 0 ? brow : -1; gain[t] = best > 0 ? best : 0; }
    if (best <= 0 || brow < 0 || brow >= N) return;
    const long long o1 = offsets[brow + 1];
    for (long long e = offsets[brow] + tid; e < o1; e += 256) {
        const unsigned v = (unsigned)nbr[e];
        if ((long long)v < N) covered[v] = 1;
    }
}

long long mc_chunks(long long N) { return (N + MC_ROWS - 1) / MC_ROWS; }

int pb_check_pool(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D, float radius2,
                  const void* dev_scratch) {
    ALINK_REQUIRE(dev_x && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_li || (dev_r && dev_ri), ALINK_EINVAL, "the pair form needs dev_r and dev_ri beside dev_li");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d", D, RB_MAX_D);
    ALINK_REQUIRE(radius2 > 0.f && radius2 < INFINITY, ALINK_EINVAL, "radius2=%g must be finite and > 0", (double)radius2);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    return ALINK_OK;
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

size_t alink_ball_scratch_bytes(int64_t N, int D) {
    if (N <= 0 || N >= (1ll << 31) || D <= 0 || D > RB_MAX_D) return 0;
    return 2 * pt_align((size_t)N * 4);
}

int alink_ball_count(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                     const int32_t* dev_group, float radius2, int32_t* dev_deg, float* dev_t_other, int32_t* dev_j_other,
                     void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_deg || dev_t_other || dev_j_other, ALINK_EINVAL, "NULL argument: every output is NULL");
    ALINK_REQUIRE(dev_group || (!dev_t_other && !dev_j_other), ALINK_EINVAL, "dev_t_other / dev_j_other need dev_group");
    const int rc = pb_check_pool(dev_x, dev_r, dev_li, dev_ri, N, D, radius2, dev_scratch);
    if (rc != ALINK_OK) return rc;
    DeviceGuard dg(device_of_pointer(dev_x));
    const RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    const PbOut o{radius2, dev_deg, dev_t_other, dev_j_other, nullptr, 0, nullptr, nullptr};
    float* xnorm = (float*)dev_scratch;
    if (dev_t_other || dev_j_other) pb_dispatch<PB_OTHER>(t, N, dev_group, o, xnorm, (hipStream_t)stream);
    else pb_dispatch<PB_DEGREE>(t, N, dev_group, o, xnorm, (hipStream_t)stream);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

int alink_ball_fill(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                    const int32_t* dev_group, float radius2, const int64_t* dev_offsets, int64_t E, int32_t* dev_nbr,
                    int32_t* dev_mismatch, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_offsets && dev_nbr && dev_mismatch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(E >= 0, ALINK_EINVAL, "E=%lld is negative", (long long)E);
    const int rc = pb_check_pool(dev_x, dev_r, dev_li, dev_ri, N, D, radius2, dev_scratch);
    if (rc != ALINK_OK) return rc;
    DeviceGuard dg(device_of_pointer(dev_x));
    const RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    float* xnorm = (float*)dev_scratch;
    int32_t* flag = (int32_t*)((char*)dev_scratch + pt_align((size_t)N * 4));
    // (PbOut.deg carries dev_mismatch to the final launch)
    const PbOut o{radius2, dev_mismatch, nullptr, nullptr, (const long long*)dev_offsets, (long long)E, dev_nbr, flag};
    pb_dispatch<PB_FILL>(t, N, dev_group, o, xnorm, (hipStream_t)stream);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

size_t alink_max_coverage_scratch_bytes(int64_t N, int k) {
    if (N <= 0 || N >= (1ll << 31) || k < 1) return 0;
    return 2 * pt_align((size_t)mc_chunks(N) * 4);
}

int alink_max_coverage(const int64_t* dev_offsets, const int32_t* dev_nbr, int64_t N, const int32_t* dev_seed, int64_t S, int k,
                       uint8_t* dev_covered, int32_t* dev_picks, int32_t* dev_gain, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_offsets && dev_nbr && dev_covered && dev_picks && dev_gain && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(k >= 1, ALINK_EINVAL, "k=%d must be at least 1", k);
    ALINK_REQUIRE(S >= 0 && S < (1ll << 31), ALINK_EINVAL, "S=%lld outside 0..2^31-1", (long long)S);
    ALINK_REQUIRE(S == 0 || dev_seed, ALINK_EINVAL, "NULL argument: S=%lld seeds without dev_seed", (long long)S);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_offsets));
    hipStream_t st = (hipStream_t)stream;
    const long long* off = (const long long*)dev_offsets;
    const long long C = mc_chunks(N);
    int32_t* cdeg = (int32_t*)dev_scratch;
    int32_t* crow = (int32_t*)((char*)dev_scratch + pt_align((size_t)C * 4));
    if (S > 0)
        hipLaunchKernelGGL(mc_seed_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, off, dev_nbr, (long long)N, dev_seed, (long long)S,
                           dev_covered);
    for (int t = 0; t < k; ++t) {
        hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)C), dim3(256), 0, st, off, dev_nbr, (long long)N, dev_covered, cdeg, crow);
        hipLaunchKernelGGL(mc_pick_kernel, dim3(1), dim3(256), 0, st, off, dev_nbr, (long long)N, cdeg, crow, C, t, dev_picks, dev_gain,
                           dev_covered);
    }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
