// kmeans.hip — Lloyd's k-means on device: the assignment of N pool rows to K centres and the update of the centres, T times,
// then one last assignment.  The clustering family of batch strategies (k-means sampling, the baseline of Ash et al. 2020, and
// the diverse mini-batch of Zhdanov 2019: a-link_amd/cluster.py) needs it; badge.kmeans_pp_device supplies the seeds.
// include/alink_hip.h (alink_kmeans) states the rule in full.
//
// What bounds it: the assignment is an (N x D)(D x K) product with an argmin epilogue — the selection side's first kernel on the
// matrix cores, the tile product of pool_tile.h (which describes the geometry and why x . c is ONE ascending fmaf chain whatever
// tile a row or a centre falls in).  The (N x K) product never exists: a wave keeps the running (score, centre) minimum of its
// 32 rows in registers across ALL centre tiles.
//
// Launches, all on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative launch, no grid
// barrier, no floating-point atomics, no atomics at all, nothing read back).  Per pass t = 0 .. T:
//   pt_norm_kernel    (pool_tile.h) over the centres as a row table: |c_j|^2 of this pass, one wave per centre, in the summation
//                     order of batch_rows.h
//   km_assign_kernel  pt_product per tile of 128 centres — a pair-form pool against row-table centres, each with a load width of
//                     its own.  In a lane the 16 centres of a block come in ascending order, so a strict `<` keeps the lower
//                     centre among ties; the two halves of a row meet once at the end in one exchange with lane ^ 32 (ties to the
//                     lower index).  A padded centre has |c|^2 = +inf and a padded row is dropped: padding never wins.  Writes a_n
//                     into scratch.
//   km_dist_kernel    the light pass: d2_n = |x_n - c_(a_n)|^2 in batch_rows.h's difference form and order, `changed` against the
//                     previous pass's dev_assign (then overwritten by the same wave: no other workgroup reads that row), and the
//                     float64 inertia, one partial per workgroup over its contiguous chunk of rows.
//   km_reduce_kernel  one workgroup: the partials in ascending order -> inertia[t], changed[t]
//   km_accum_kernel   grid (K, S, ceil(D / 256)), one wave each: wave (j, s, b) scans slice s of dev_assign in ascending row order
//                     and adds w_n x_n of cluster j's rows into float64, four columns per lane; block 0 also counts the rows, sums
//                     the weights and keeps the slice's nearest row.  S is a function of (N, K) alone (pt_slices).
//   km_final_kernel   one workgroup per centre: the S partials in ascending s, one float64 division, one rounding to float32 (t < T),
//                     or counts / wsum / nearest (t = T, where km_accum_kernel runs without the column sums).
// Hazards.  Every kernel reads only what an EARLIER launch wrote, with two exceptions that stay inside one wave: km_dist_kernel
// reads and rewrites dev_assign[n] and km_final_kernel leaves an empty cluster's centre as it is.  So nothing here needs a second
// buffer: the centres are updated in place by km_final_kernel, which reads none of them, and km_assign_kernel writes a scratch
// vector, not dev_assign, which km_dist_kernel still needs for `changed`.
//
// Every float64 sum runs in an order fixed by (N, K) and the assignment alone: results are bit-identical from run to run.
// Measured (one MI355X, K = 1,024): km_assign_kernel 647 us at 200,000 x 128 (81 TFLOP/s, 52 % of the 157.3 TFLOP/s
// f32 matrix peak), 2,794 us at 200,000 pairs x 512 in the pair form (75 TFLOP/s); km_accum_kernel 277 / 300 us, all of it the
// scan of the assignment vector (259 us without the column sums); an iteration 0.99 / 3.19 ms.  The exact-f32 GEMM + argmin the
// library could do before takes 1.43 / 3.53 ms for the assignment alone.
// Not built: the early return of passes after a pass with changed = 0 (they run, and give what they must: the same again).
#include "pool_tile.h"

namespace alink {
namespace {

constexpr int KM_MAX_K = 8192;
constexpr int KM_MAX_GRID = 2048;          // workgroups (= partials) of the light pass
constexpr int KM_PASS_ROWS = 2;            // rows per wave and pass of the light pass
constexpr int KM_WG_PASS = 4 * KM_PASS_ROWS;
constexpr unsigned long long KM_NO_KEY = ~0ull;

__device__ __forceinline__ double km_weight(const float* __restrict__ w, long long n) {
    if (!w) return 1.0;
    const float v = w[n];
    return (v > 0.f && v < INFINITY) ? (double)v : 0.0;
}

__host__ __device__ __forceinline__ long long km_chunk_rows(long long N) {
    const long long per = (long long)KM_MAX_GRID * KM_WG_PASS;
    return KM_WG_PASS * ((N + per - 1) / per);
}

template <bool PAIR, bool VEC, bool VECC>
__global__ __launch_bounds__(256) void km_assign_kernel(const RbRows t, long long N, const float* __restrict__ centres,
                                                        const float* __restrict__ cnorm, int K, int32_t* __restrict__ anew) {
    __shared__ float sX[PT_DC * PT_LD];
    __shared__ float sC[PT_DC * PT_LD];
    __shared__ __attribute__((aligned(16))) float sN[PT_TK];
    const int D = t.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const long long n0 = (long long)blockIdx.x * PT_TN;
    const RbRows ct{centres, nullptr, nullptr, nullptr, D};
    const int srow = tid & 127;            // the tile row this thread stages (pool_tile.h)
    const long long xn = n0 + srow;
    const bool xhave = xn < N;

    float best = INFINITY;                 // a score wins by `<` alone: neither NaN nor +inf ever does
    int bestj = -1;
    for (int k0 = 0; k0 < K; k0 += PT_TK) {
        const int nblk = min(4, (K - k0 + 31) >> 5);      // MFMA row blocks of this tile that hold a centre (uniform)
        const bool chave = k0 + srow < K;
        f32x16 acc[4];
        pt_product<PAIR, VEC, false, VECC>(t, xn, xhave, ct, k0 + srow, chave, nblk, sX, sC, acc,
                                           [&](int i) { sN[i] = k0 + i < K ? cnorm[k0 + i] : INFINITY; });
        // the tile's scores against the running minimum: in a lane the centres come in ascending order
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nblk) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 cn = *(const float4*)(sN + b * 32 + 8 * g + 4 * hh);
                    const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float s = __builtin_fmaf(-2.f, acc[b][4 * g + i], cnv[i]);
                        if (s < best) { best = s; bestj = k0 + b * 32 + 8 * g + 4 * hh + i; }
                    }
                }
            }
        }
    }
    const float ob = __shfl_xor(best, 32, 64);
    const int oj = __shfl_xor(bestj, 32, 64);
    if (oj >= 0 && (bestj < 0 || ob < best || (ob == best && oj < bestj))) { best = ob; bestj = oj; }
    const long long n = n0 + wave * 32 + l31;
    if (hh == 0 && n < N) anew[n] = bestj;
}

// the light pass over a contiguous chunk of rows per workgroup: d2, changed, the inertia partial
template <bool PAIR, bool VEC, bool VECC>
__global__ __launch_bounds__(256) void km_dist_kernel(const RbRows t, long long N, long long chunk, const float* __restrict__ centres,
                                                      const float* __restrict__ weight, const int32_t* __restrict__ anew,
                                                      int32_t* __restrict__ assign, float* __restrict__ d2_out, int first,
                                                      double* __restrict__ part_inertia, int32_t* __restrict__ part_changed) {
    __shared__ double s_sum[4];
    __shared__ int s_chg[4];
    constexpr int NR = KM_PASS_ROWS;
    const int D = t.D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
    double isum = 0.0;                                     // this wave's rows, in ascending order
    int chg = 0;
    for (long long n0 = r0 + wave * NR; n0 < r1; n0 += KM_WG_PASS) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const long long n = n0 + j;
            if (n >= r1) continue;                         // (uniform over the wave)
            const int a = anew[n];
            const int old = first ? -1 : assign[n];
            float d = __builtin_nanf("");
            if (a >= 0) {
                const RbRow r = rb_row<PAIR>(t, n);
                const RbRow c{centres + (size_t)a * D, nullptr};
                float s = 0.f;
                for (int e0 = 4 * lane; e0 < D; e0 += 256) s = rb_acc(s, rb_quad<PAIR, VEC>(r, e0, D), rb_quad<false, VECC>(c, e0, D));
                d = rb_wave_sum(s);
                const double w = km_weight(weight, n);
                if (w > 0.0) isum += w * (double)d;
            }
            chg += a != old;
            if (lane == 0) {
                assign[n] = a;
                d2_out[n] = d;
            }
        }
    }
    if (lane == 0) { s_sum[wave] = isum; s_chg[wave] = chg; }   // (every lane of a wave holds the same)
    __syncthreads();
    if (threadIdx.x == 0) {
        part_inertia[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        part_changed[blockIdx.x] = s_chg[0] + s_chg[1] + s_chg[2] + s_chg[3];
    }
}

// one workgroup: thread i adds partials 8 i .. 8 i + 7 in ascending order, thread 0 the 256 totals in ascending order
__global__ __launch_bounds__(256) void km_reduce_kernel(const double* __restrict__ part_inertia, const int32_t* __restrict__ part_changed,
                                                        int nparts, int pass, double* __restrict__ inertia, int32_t* __restrict__ changed) {
    __shared__ double s_sum[256];
    __shared__ long long s_chg[256];
    double s = 0.0;
    long long c = 0;
    for (int j = 0; j < KM_MAX_GRID / 256; ++j) {
        const int p = threadIdx.x * (KM_MAX_GRID / 256) + j;
        if (p < nparts) { s += part_inertia[p]; c += part_changed[p]; }
    }
    s_sum[threadIdx.x] = s;
    s_chg[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0.0;
        c = 0;
        for (int i = 0; i < 256; ++i) { s += s_sum[i]; c += s_chg[i]; }
        if (inertia) inertia[pass] = s;
        if (changed) changed[pass] = (int32_t)c;
    }
}

// wave (j, s, b): cluster j's rows of slice s in ascending order; columns 256 b + 4 lane .. + 3 in float64
template <bool PAIR, bool VEC>
__global__ __launch_bounds__(64) void km_accum_kernel(const RbRows t, long long N, long long slice, int S, const int32_t* __restrict__ assign,
                                                      const float* __restrict__ weight, const float* __restrict__ d2, int sums,
                                                      double* __restrict__ psum, double* __restrict__ pw, int32_t* __restrict__ pcount,
                                                      unsigned long long* __restrict__ pkey) {
    const int D = t.D;
    const int lane = threadIdx.x, j = blockIdx.x, s = blockIdx.y;
    const int e0 = 256 * (int)blockIdx.z + 4 * lane;
    const bool stats = blockIdx.z == 0;
    const bool cols = sums && e0 < D;
    const long long r0 = (long long)s * slice, r1 = r0 + slice < N ? r0 + slice : N;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, wsum = 0.0;
    int count = 0;
    unsigned long long key = KM_NO_KEY;
    for (long long base = r0; base < r1; base += PT_SLICE_ALIGN) {
        unsigned long long m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long n = base + 64 * u + lane;
            const bool mine = n < r1 && assign[n] == j;
            m[u] = __ballot(mine);
            if (mine && stats) {
                const unsigned long long k = ((unsigned long long)__float_as_uint(d2[n]) << 32) | (unsigned long long)n;
                key = k < key ? k : key;                   // d2 >= 0: its bits order as the values do; ties to the lower row
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned long long mm = m[u];
            count += __popcll(mm);
            while (mm) {                                   // (uniform over the wave)
                const long long n = base + 64 * u + (__ffsll((long long)mm) - 1);
                mm &= mm - 1;
                const double w = km_weight(weight, n);
                if (!(w > 0.0)) continue;
                wsum += w;
                if (cols) {
                    const float4 x = rb_quad<PAIR, VEC>(rb_row<PAIR>(t, n), e0, D);
                    a0 += w * (double)x.x; a1 += w * (double)x.y; a2 += w * (double)x.z; a3 += w * (double)x.w;
                }
            }
        }
    }
    const size_t slot = (size_t)j * S + s;
    if (cols) {
        double* o = psum + slot * D;
        o[e0] = a0;
        if (e0 + 1 < D) o[e0 + 1] = a1;
        if (e0 + 2 < D) o[e0 + 2] = a2;
        if (e0 + 3 < D) o[e0 + 3] = a3;
    }
    if (stats) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long k = __shfl_xor(key, o, 64);
            key = k < key ? k : key;
        }
        if (lane == 0) { pw[slot] = wsum; pcount[slot] = count; pkey[slot] = key; }
    }
}

// one workgroup per centre: the slices' partials in ascending order
__global__ __launch_bounds__(256) void km_final_kernel(int D, int S, int last, const double* __restrict__ psum, const double* __restrict__ pw,
                                                       const int32_t* __restrict__ pcount, const unsigned long long* __restrict__ pkey,
                                                       float* __restrict__ centres, int32_t* __restrict__ counts, double* __restrict__ wsum_out,
                                                       int32_t* __restrict__ nearest) {
    const int j = blockIdx.x;
    const size_t slot = (size_t)j * S;
    double w = 0.0;
    for (int s = 0; s < S; ++s) w += pw[slot + s];
    if (!last) {
        if (!(w > 0.0)) return;                            // no weight: the centre stays
        for (int d = threadIdx.x; d < D; d += 256) {
            double x = 0.0;
            for (int s = 0; s < S; ++s) x += psum[(slot + s) * D + d];
            centres[(size_t)j * D + d] = (float)(x / w);
        }
        return;
    }
    if (threadIdx.x == 0) {
        int c = 0;
        unsigned long long key = KM_NO_KEY;
        for (int s = 0; s < S; ++s) {
            c += pcount[slot + s];
            key = pkey[slot + s] < key ? pkey[slot + s] : key;
        }
        if (counts) counts[j] = c;
        if (wsum_out) wsum_out[j] = w;
        if (nearest) nearest[j] = key == KM_NO_KEY ? -1 : (int32_t)(key & 0xffffffffull);
    }
}

struct KmScratch {
    int32_t* anew;
    float* d2;
    float* cnorm;
    double* part_inertia;
    int32_t* part_changed;
    double* pw;
    int32_t* pcount;
    unsigned long long* pkey;
    double* psum;
    size_t bytes;
};
KmScratch km_carve(char* base, long long N, int D, int K) {
    long long slice;
    const size_t S = (size_t)pt_slices(N, K, &slice);
    KmScratch s;
    size_t o = 0;
    auto take = [&](size_t b) { char* p = base + o; o += pt_align(b); return p; };
    s.anew = (int32_t*)take((size_t)N * 4);
    s.d2 = (float*)take((size_t)N * 4);
    s.cnorm = (float*)take((size_t)K * 4);
    s.part_inertia = (double*)take((size_t)KM_MAX_GRID * 8);
    s.part_changed = (int32_t*)take((size_t)KM_MAX_GRID * 4);
    s.pw = (double*)take((size_t)K * S * 8);
    s.pcount = (int32_t*)take((size_t)K * S * 4);
    s.pkey = (unsigned long long*)take((size_t)K * S * 8);
    s.psum = (double*)take((size_t)K * S * D * 8);
    s.bytes = o;
    return s;
}

struct KmArgs {
    const float* weight;
    float* centres;
    int K, iters;
    int32_t* assign;
    float* d2;
    double* inertia;
    int32_t* changed;
    int32_t* counts;
    double* wsum;
    int32_t* nearest;
};

template <bool PAIR, bool VEC, bool VECC>
void km_enqueue(const RbRows& t, long long N, const KmArgs& a, char* scratch, hipStream_t st) {
    const int D = t.D, K = a.K;
    const KmScratch s = km_carve(scratch, N, D, K);
    float* d2 = a.d2 ? a.d2 : s.d2;
    long long slice;
    const int S = pt_slices(N, K, &slice);
    const long long chunk = km_chunk_rows(N);
    const unsigned dgrid = (unsigned)((N + chunk - 1) / chunk);            // <= KM_MAX_GRID
    const unsigned agrid = (unsigned)((N + PT_TN - 1) / PT_TN);
    const bool stats = a.counts || a.wsum || a.nearest;
    const RbRows ct{a.centres, nullptr, nullptr, nullptr, D};             // the centres as a row table
    for (int pass = 0; pass <= a.iters; ++pass) {
        const bool last = pass == a.iters;
        hipLaunchKernelGGL((pt_norm_kernel<false, VECC>), dim3((K + 3) / 4), dim3(256), 0, st, ct, (long long)K, s.cnorm);
        hipLaunchKernelGGL((km_assign_kernel<PAIR, VEC, VECC>), dim3(agrid), dim3(256), 0, st, t, N, a.centres, s.cnorm, K, s.anew);
        hipLaunchKernelGGL((km_dist_kernel<PAIR, VEC, VECC>), dim3(dgrid), dim3(256), 0, st, t, N, chunk, a.centres, a.weight, s.anew,
                           a.assign, d2, pass == 0 ? 1 : 0, s.part_inertia, s.part_changed);
        if (a.inertia || a.changed)
            hipLaunchKernelGGL(km_reduce_kernel, dim3(1), dim3(256), 0, st, s.part_inertia, s.part_changed, (int)dgrid, pass, a.inertia,
                               a.changed);
        if (last && !stats) break;
        hipLaunchKernelGGL((km_accum_kernel<PAIR, VEC>), dim3(K, S, last ? 1 : (D + 255) / 256), dim3(64), 0, st, t, N, slice, S, a.assign,
                           a.weight, d2, last ? 0 : 1, s.psum, s.pw, s.pcount, s.pkey);
        hipLaunchKernelGGL(km_final_kernel, dim3(K), dim3(256), 0, st, D, S, last ? 1 : 0, s.psum, s.pw, s.pcount, s.pkey, a.centres,
                           a.counts, a.wsum, a.nearest);
    }
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

size_t alink_kmeans_scratch_bytes(int64_t N, int D, int K) {
    if (N <= 0 || N >= (1ll << 31) || D <= 0 || D > RB_MAX_D || K <= 0 || K > KM_MAX_K) return 0;
    return km_carve(nullptr, N, D, K).bytes;
}

int alink_kmeans(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                 const float* dev_weight, float* dev_centres, int K, int iters, int32_t* dev_assign, float* dev_d2, double* dev_inertia,
                 int32_t* dev_changed, int32_t* dev_counts, double* dev_wsum, int32_t* dev_nearest, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_x && dev_centres && dev_assign && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_li || (dev_r && dev_ri), ALINK_EINVAL, "the pair form needs dev_r and dev_ri beside dev_li");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d", D, RB_MAX_D);
    ALINK_REQUIRE(K >= 1 && K <= KM_MAX_K, ALINK_EINVAL, "K=%d outside 1..%d", K, KM_MAX_K);
    ALINK_REQUIRE(iters >= 0, ALINK_EINVAL, "iters=%d must be >= 0", iters);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_x));
    RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    const KmArgs a{dev_weight, dev_centres, K, iters, dev_assign, dev_d2, dev_inertia, dev_changed, dev_counts, dev_wsum, dev_nearest};
    hipStream_t st = (hipStream_t)stream;
    const bool pair = dev_li != nullptr;
    const bool vec = pt_vec(t);
    const bool vecc = D % 4 == 0 && ((uintptr_t)dev_centres & 15) == 0;
    char* sc = (char*)dev_scratch;
#define KM_GO(P, V, C) km_enqueue<P, V, C>(t, N, a, sc, st)
    if (pair) {
        if (vec) { if (vecc) KM_GO(true, true, true); else KM_GO(true, true, false); }
        else { if (vecc) KM_GO(true, false, true); else KM_GO(true, false, false); }
    } else {
        if (vec) { if (vecc) KM_GO(false, true, true); else KM_GO(false, true, false); }
        else { if (vecc) KM_GO(false, false, true); else KM_GO(false, false, false); }
    }
#undef KM_GO
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
