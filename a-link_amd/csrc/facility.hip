// facility.hip — facility-location batches: the k rows of a pool that minimise sum_n min_(s in S) |x_n - x_s|^2, chosen by the
// greedy of largest gain, plain (every row a candidate) or stochastic (a sample of R candidates per pick: Mirzasoleiman et al.
// 2015, "Lazier Than Lazy Greedy").  The selection rule of FASS (Wei, Iyer & Bilmes 2015), of CRAIG's coresets and of the SIMILAR
// family (a-link_amd/facility.py).  include/alink_hip.h (alink_facility_gains) states the rule in full.
//
// What bounds it: per pick an (R x D)(D x N) product on the f32 matrix cores — the tile product of pool_tile.h — with a SUM
// epilogue.  km_assign_kernel turned round: the workgroup's 128 rows of pt_product are 128 CANDIDATES, gathered through dev_cand,
// and the pool walks past as the tile's candidates.  Lane (l, h) of a wave holds for its own candidate the 16 pool rows
// 8 g + 4 h + i of each block, so the sum over pool rows is lane-local: one float64 accumulator per block in place of k-means'
// running minimum, the two half-lanes of a candidate combined once at the end.  The (N x R) scores never reach memory.
//
// fl_w is the ONE place the score is formed, in the gains and in the cover kernel: t = fmaf(-2, dot, xn_a + xn_b) — probcover.hip's
// pb_score restated — clamped below at 0, a NaN kept.  The dot is one ascending fmaf chain whichever operand a row is
// (pool_tile.h) and the addition commutes: w(n, c) in the gains pass and w(n, s) in the cover pass are the same bits, so after
// a pick p cur_p <= w(p, p) and p's gain is exactly 0 from then on.
//
// Launches, all on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative launch, no grid
// barrier, no atomics, nothing read back):
//   pt_norm_kernel   (pool_tile.h) |x_n|^2 of every row, once per call
//   fl_gains_kernel  grid (ceil(R / 128) candidate tiles, S slabs of pool rows); side() stages the pool tile's norms and cur — a
//                    padded row, or one whose norm is not finite, with cur = -inf: its term max(0, cur - w) is 0 without a branch.
//                    Each workgroup writes its 128 partial gains to part[slab][position] with plain stores.
//   fl_sum_kernel    (alink_facility_gains) gain[r] = the slabs' partials in ascending order
//   fl_pick_kernel   (alink_facility_select) ONE workgroup: the same sums, the position of largest gain by `>` from 0, ties to the
//                    lower position; writes dev_picks[t], dev_gain[t]
//   fl_cover_kernel  workgroup = 128 pool rows, the selected rows walk past in tiles of 128 gathered through dev_sel; the running
//                    minimum stays in registers and cur is updated in place
// Hazards between the three launches of a pick: fl_gains_kernel reads cur and writes part; fl_pick_kernel reads part and writes
// picks[t], gain[t]; fl_cover_kernel reads picks[t] and the pool, and reads and writes cur — each row of cur by the one workgroup
// that owns it, which no other workgroup of that launch reads.  The next pick's gains pass overwrites part only after the pick
// launch that read it.  So one part buffer and cur in place suffice.
// S (fl_slabs) is a function of (N, R) alone and the slab length a multiple of 128; every float64 sum runs in an order fixed by
// (N, R): results are bit-identical from run to run and exact wherever the terms are integers.
// Measured: DESIGN.md §9.  Not built: lazy-greedy bounds, row weights, a cosine metric, the cover of pick t fused into the gains
// pass of pick t + 1, several ranks' pools in one call.
#include "pool_tile.h"

namespace alink {
namespace {

constexpr long long FL_TARGET_WGS = 1024;  // workgroups the gains grid aims for: four per CU

// the score both kernels share: ProbCover's t, clamped below at 0; a NaN stays NaN
__device__ __forceinline__ float fl_w(float dot, float xn_a, float xn_b) {
    const float t = __builtin_fmaf(-2.f, dot, xn_a + xn_b);
    return t < 0.f ? 0.f : t;
}

// slabs of pool rows of the gains grid: a function of (N, R) alone.  *len = rows of a slab (a multiple of 128), -> their number
inline long long fl_slabs(long long N, long long R, long long* len) {
    const long long tiles = (R + PT_TN - 1) / PT_TN;
    long long S = (FL_TARGET_WGS + tiles - 1) / tiles;
    if (S < 1) S = 1;
    long long L = (N + S - 1) / S;
    L = (L + PT_TK - 1) / PT_TK * PT_TK;
    *len = L;
    return (N + L - 1) / L;
}

// index of candidate position r: -1 where the position or the index is outside its range
__device__ __forceinline__ long long fl_candidate(const int32_t* __restrict__ cand, long long r, long long R, long long N) {
    if (r >= R) return -1;
    const long long c = cand ? (long long)cand[r] : r;
    return (c >= 0 && c < N) ? c : -1;
}

// Two waves per SIMD, as pb_tile_kernel has.
template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256, 2) void fl_gains_kernel(const RbRows t, long long N, const float* __restrict__ xnorm,
                                                           const float* __restrict__ cur, const int32_t* __restrict__ cand, long long R,
                                                           long long slab, long long rpad, double* __restrict__ part) {
    __shared__ float sX[PT_DC * PT_LD];
    __shared__ float sC[PT_DC * PT_LD];
    __shared__ __attribute__((aligned(16))) float sN[PT_TK];
    __shared__ __attribute__((aligned(16))) float sU[PT_TK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const long long r0 = (long long)blockIdx.x * PT_TN;
    const long long j0 = (long long)blockIdx.y * slab, j1 = j0 + slab < N ? j0 + slab : N;
    const int srow = tid & 127;            // the tile row this thread stages (pool_tile.h): a candidate
    const long long sc = fl_candidate(cand, r0 + srow, R, N);

    // this lane's candidate and its norm
    const long long rl = r0 + wave * 32 + l31;
    const long long cl = fl_candidate(cand, rl, R, N);
    const float xnn = cl >= 0 ? xnorm[cl] : 0.f;

    double a[4] = {0.0, 0.0, 0.0, 0.0};    // per MFMA block: this lane's pool rows in ascending order
    for (long long k0 = j0; k0 < j1; k0 += PT_TK) {
        const long long left = j1 - k0;
        const int nblk = left >= PT_TK ? 4 : (int)((left + 31) >> 5);      // MFMA row blocks of this tile that hold a pool row (uniform)
        const long long pn = k0 + srow;
        f32x16 acc[4];
        pt_product<PAIR, VEC, PAIR, VEC>(t, sc < 0 ? 0 : sc, sc >= 0, t, pn, pn < j1, nblk, sX, sC, acc, [&](int i) {
            const long long j = k0 + i;
            const float nj = j < j1 ? xnorm[j] : INFINITY;
            const bool ok = nj < INFINITY && nj > -INFINITY;               // (false for NaN)
            sN[i] = ok ? nj : 0.f;
            sU[i] = ok ? cur[j] : -INFINITY;                               // no term: max(0, -inf - w) = 0
        });
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nblk) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 cn = *(const float4*)(sN + b * 32 + 8 * g + 4 * hh);
                    const float4 cu = *(const float4*)(sU + b * 32 + 8 * g + 4 * hh);
                    const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
                    const float cuv[4] = {cu.x, cu.y, cu.z, cu.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float d = cuv[i] - fl_w(acc[b][4 * g + i], xnn, cnv[i]);
                        a[b] += (double)(d > 0.f ? d : 0.f);               // (a NaN on either side: 0)
                    }
                }
            }
        }
    }
    double s = ((a[0] + a[1]) + a[2]) + a[3];
    const double o = __shfl_xor(s, 32, 64);                                // the two halves of a candidate meet: lower half first
    s = s + o;
    const bool live = cl >= 0 && xnn < INFINITY && xnn > -INFINITY;
    if (hh == 0) part[(long long)blockIdx.y * rpad + rl] = live ? s : 0.0;  // (rl < rpad = 128 gridDim.x)
}

// gain[r] = the slabs' partials in ascending order
__global__ __launch_bounds__(256) void fl_sum_kernel(const double* __restrict__ part, long long R, long long rpad, int S,
                                                     double* __restrict__ gain) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    double g = 0.0;
    for (int s = 0; s < S; ++s) g += part[(long long)s * rpad + r];
    gain[r] = g;
}

// ONE workgroup: every position's gain as fl_sum_kernel forms it, the largest by `>` from 0, ties to the lower position
__global__ __launch_bounds__(256) void fl_pick_kernel(const double* __restrict__ part, long long R, long long rpad, int S,
                                                      const int32_t* __restrict__ cand, int t, int32_t* __restrict__ picks,
                                                      double* __restrict__ gain) {
    __shared__ double sg[256];
    __shared__ long long sp[256];
    const int tid = threadIdx.x;
    double best = 0.0;
    long long bpos = -1;
    for (long long r = tid; r < R; r += 256) {             // a thread's positions ascend: `>` keeps the lower one
        double g = 0.0;
        for (int s = 0; s < S; ++s) g += part[(long long)s * rpad + r];
        if (g > best) { best = g; bpos = r; }
    }
    sg[tid] = best; sp[tid] = bpos;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {                                     // (gain descending, position ascending): the same winner in any order
            const double g = sg[tid + w];
            const long long p = sp[tid + w];
            if (g > sg[tid] || (g == sg[tid] && g > 0.0 && p < sp[tid])) { sg[tid] = g; sp[tid] = p; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        best = sg[0]; bpos = sp[0];
        const bool won = best > 0.0 && bpos >= 0;
        picks[t] = won ? (cand ? cand[bpos] : (int32_t)bpos) : -1;
        gain[t] = won ? best : 0.0;
    }
}

template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256, 2) void fl_cover_kernel(const RbRows t, long long N, const float* __restrict__ xnorm,
                                                           float* __restrict__ cur, const int32_t* __restrict__ sel, long long S) {
    __shared__ float sX[PT_DC * PT_LD];
    __shared__ float sC[PT_DC * PT_LD];
    __shared__ __attribute__((aligned(16))) float sN[PT_TK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const long long n0 = (long long)blockIdx.x * PT_TN;
    const int srow = tid & 127;            // the tile row this thread stages (pool_tile.h): a pool row
    const long long xn = n0 + srow;
    const bool xhave = xn < N;

    // this lane's row: a row past the pool, or whose norm is not finite, keeps its cur
    const long long n = n0 + wave * 32 + l31;
    float xnn = 0.f, cur0 = 0.f;
    bool live = false;
    if (n < N) {
        xnn = xnorm[n];
        cur0 = cur[n];
        live = xnn < INFINITY && xnn > -INFINITY;
    }
    float m = cur0;                        // the running minimum by `<`: a NaN neither enters nor leaves
    for (long long k0 = 0; k0 < S; k0 += PT_TK) {
        const long long left = S - k0;
        const int nblk = left >= PT_TK ? 4 : (int)((left + 31) >> 5);      // MFMA row blocks of this tile that hold a selected row (uniform)
        long long sj = k0 + srow < S ? (long long)sel[k0 + srow] : -1;
        if (sj >= N) sj = -1;
        f32x16 acc[4];
        pt_product<PAIR, VEC, PAIR, VEC>(t, xn, xhave, t, sj < 0 ? 0 : sj, sj >= 0, nblk, sX, sC, acc, [&](int i) {
            long long j = k0 + i < S ? (long long)sel[k0 + i] : -1;
            if (j >= N) j = -1;
            const float nj = j >= 0 ? xnorm[j] : INFINITY;
            sN[i] = (nj < INFINITY && nj > -INFINITY) ? nj : INFINITY;     // +inf: w is +inf or NaN, which is never `<`
        });
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nblk) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 cn = *(const float4*)(sN + b * 32 + 8 * g + 4 * hh);
                    const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float w = fl_w(acc[b][4 * g + i], xnn, cnv[i]);
                        m = w < m ? w : m;
                    }
                }
            }
        }
    }
    const float om = __shfl_xor(m, 32, 64);                // the two halves of a row meet
    m = om < m ? om : m;
    if (hh == 0 && live && m < cur0) cur[n] = m;
}

template <bool PAIR, bool VEC>
void fl_norms(const RbRows& t, long long N, float* xnorm, hipStream_t st) {
    hipLaunchKernelGGL((pt_norm_kernel<PAIR, VEC>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, t, N, xnorm);
}

struct FlPlan {
    long long slab, rpad;
    int S;
    unsigned tiles;
};
FlPlan fl_plan(long long N, long long R) {
    FlPlan p;
    p.S = (int)fl_slabs(N, R, &p.slab);
    p.tiles = (unsigned)((R + PT_TN - 1) / PT_TN);
    p.rpad = (long long)p.tiles * PT_TN;
    return p;
}

template <bool PAIR, bool VEC>
void fl_gains(const RbRows& t, long long N, const float* xnorm, const float* cur, const int32_t* cand, long long R, const FlPlan& p,
              double* part, hipStream_t st) {
    hipLaunchKernelGGL((fl_gains_kernel<PAIR, VEC>), dim3(p.tiles, (unsigned)p.S), dim3(256), 0, st, t, N, xnorm, cur, cand, R, p.slab,
                       p.rpad, part);
}

template <bool PAIR, bool VEC>
void fl_cover(const RbRows& t, long long N, const float* xnorm, float* cur, const int32_t* sel, long long S, hipStream_t st) {
    hipLaunchKernelGGL((fl_cover_kernel<PAIR, VEC>), dim3((unsigned)((N + PT_TN - 1) / PT_TN)), dim3(256), 0, st, t, N, xnorm, cur, sel, S);
}

template <bool PAIR, bool VEC>
void fl_select(const RbRows& t, long long N, float* xnorm, float* cur, const int32_t* cand, long long R, int k, const FlPlan& p,
               double* part, int32_t* picks, double* gain, hipStream_t st) {
    fl_norms<PAIR, VEC>(t, N, xnorm, st);
    for (int i = 0; i < k; ++i) {
        const int32_t* ci = cand ? cand + (size_t)i * (size_t)R : nullptr;
        fl_gains<PAIR, VEC>(t, N, xnorm, cur, ci, R, p, part, st);
        hipLaunchKernelGGL(fl_pick_kernel, dim3(1), dim3(256), 0, st, part, R, p.rpad, p.S, ci, i, picks, gain);
        fl_cover<PAIR, VEC>(t, N, xnorm, cur, picks + i, 1, st);
    }
}

size_t fl_part_offset(long long N) { return pt_align((size_t)N * 4); }

int fl_check_pool(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                  const float* dev_cur, const void* dev_scratch) {
    ALINK_REQUIRE(dev_x && dev_cur && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_li || (dev_r && dev_ri), ALINK_EINVAL, "the pair form needs dev_r and dev_ri beside dev_li");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d", D, RB_MAX_D);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    return ALINK_OK;
}

int fl_check_candidates(const int32_t* dev_cand, int64_t R, int64_t N) {
    ALINK_REQUIRE(R >= 1 && R <= N, ALINK_EINVAL, "R=%lld outside 1..N=%lld", (long long)R, (long long)N);
    ALINK_REQUIRE(dev_cand || R == N, ALINK_EINVAL, "dev_cand NULL names every row: R=%lld must equal N=%lld", (long long)R, (long long)N);
    return ALINK_OK;
}

}  // namespace
}  // namespace alink

using namespace alink;

#define FL_GO(CALL)                                                                             \
    do {                                                                                        \
        const bool pair__ = t.li != nullptr, vec__ = pt_vec(t);                                 \
        if (pair__) { if (vec__) CALL(true, true); else CALL(true, false); }                    \
        else { if (vec__) CALL(false, true); else CALL(false, false); }                         \
    } while (0)

extern "C" {

size_t alink_facility_scratch_bytes(int64_t N, int D, int64_t R, int k) {
    if (N <= 0 || N >= (1ll << 31) || D <= 0 || D > RB_MAX_D || R < 1 || R > N || k < 1) return 0;
    const FlPlan p = fl_plan(N, R);
    return fl_part_offset(N) + pt_align((size_t)p.S * (size_t)p.rpad * 8);
}

int alink_facility_gains(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                         const float* dev_cur, const int32_t* dev_cand, int64_t R, double* dev_gain, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_gain, ALINK_EINVAL, "NULL argument");
    int rc = fl_check_pool(dev_x, dev_r, dev_li, dev_ri, N, D, dev_cur, dev_scratch);
    if (rc != ALINK_OK) return rc;
    rc = fl_check_candidates(dev_cand, R, N);
    if (rc != ALINK_OK) return rc;
    DeviceGuard dg(device_of_pointer(dev_x));
    hipStream_t st = (hipStream_t)stream;
    const RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    const FlPlan p = fl_plan(N, R);
    float* xnorm = (float*)dev_scratch;
    double* part = (double*)((char*)dev_scratch + fl_part_offset(N));
#define FL_CALL(P, V)                                                                   \
    do {                                                                                \
        fl_norms<P, V>(t, N, xnorm, st);                                                \
        fl_gains<P, V>(t, N, xnorm, dev_cur, dev_cand, R, p, part, st);                 \
    } while (0)
    FL_GO(FL_CALL);
#undef FL_CALL
    hipLaunchKernelGGL(fl_sum_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, part, (long long)R, p.rpad, p.S, dev_gain);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

int alink_facility_cover(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                         float* dev_cur, const int32_t* dev_sel, int64_t S, void* dev_scratch, void* stream) {
    const int rc = fl_check_pool(dev_x, dev_r, dev_li, dev_ri, N, D, dev_cur, dev_scratch);
    if (rc != ALINK_OK) return rc;
    ALINK_REQUIRE(S >= 0 && S < (1ll << 31), ALINK_EINVAL, "S=%lld outside 0..2^31-1", (long long)S);
    ALINK_REQUIRE(S == 0 || dev_sel, ALINK_EINVAL, "NULL argument: S=%lld selected rows without dev_sel", (long long)S);
    if (S == 0) return ALINK_OK;                           // nothing to cover: nothing is launched
    DeviceGuard dg(device_of_pointer(dev_x));
    hipStream_t st = (hipStream_t)stream;
    const RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    float* xnorm = (float*)dev_scratch;
#define FL_CALL(P, V)                                                                   \
    do {                                                                                \
        fl_norms<P, V>(t, N, xnorm, st);                                                \
        fl_cover<P, V>(t, N, xnorm, dev_cur, dev_sel, S, st);                           \
    } while (0)
    FL_GO(FL_CALL);
#undef FL_CALL
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

int alink_facility_select(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                          float* dev_cur, const int32_t* dev_cand, int64_t R, int k, int32_t* dev_picks, double* dev_gain,
                          void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_picks && dev_gain, ALINK_EINVAL, "NULL argument");
    int rc = fl_check_pool(dev_x, dev_r, dev_li, dev_ri, N, D, dev_cur, dev_scratch);
    if (rc != ALINK_OK) return rc;
    rc = fl_check_candidates(dev_cand, R, N);
    if (rc != ALINK_OK) return rc;
    ALINK_REQUIRE(k >= 1, ALINK_EINVAL, "k=%d must be at least 1", k);
    DeviceGuard dg(device_of_pointer(dev_x));
    hipStream_t st = (hipStream_t)stream;
    const RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    const FlPlan p = fl_plan(N, R);
    float* xnorm = (float*)dev_scratch;
    double* part = (double*)((char*)dev_scratch + fl_part_offset(N));
#define FL_CALL(P, V) fl_select<P, V>(t, N, xnorm, dev_cur, dev_cand, R, k, p, part, dev_picks, dev_gain, st)
    FL_GO(FL_CALL);
#undef FL_CALL
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
