// kmeanspp.hip — k-means++ seeding on device (Arthur & Vassilvitskii 2007), the batch rule of BADGE (Ash et al. 2020) over the
// gradient embeddings alink_head_egl writes: the first centre is the row of largest norm, every later one is drawn with
// probability proportional to its squared distance to the nearest centre so far.  The package's only SAMPLING strategy, so
// the arithmetic of the draw is pinned (include/alink_hip.h states the rule in full): d2 in float32 in the one summation
// order of batch_rows.h, weights, cumulative sums and the target u T in float64, pick = the first row whose cumulative sum
// exceeds the target.
//
// What bounds it: one pass over the pool per pick, two rows per wave at a time against the picked row in LDS — vector-ALU
// work without MFMA, bound by HBM or, for a pool the Infinity Cache holds (200,000 x 128 floats are 102 MB of its 256 MB), by
// that cache.  batch.hip's streaming pass with its max-reduction replaced by a sampled inverse CDF.
//
// Launches, all on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative launch, no grid
// barrier, no atomics, no workgroup waits on another):
//   kp_norm_kernel       only for first = -1: |x_n|^2 of every row, one (value, index) argmax candidate per workgroup
//   kp_step_kernel x k-1 launch s resolves pick s in its prologue and folds it into d2 in its body (the last pick needs no body).
//                        Workgroup g owns the CONTIGUOUS rows [g c, (g + 1) c), c = 8 ceil(N / 16384): a function of N alone, a
//                        multiple of the 8 rows a workgroup takes per pass, at most KP_MAX_GRID chunks.
//                        Prologue, by EVERY workgroup redundantly: the previous launch's per-chunk float64 sums -> their
//                        prefix in ascending chunk order (thread i takes chunks 8 i .. 8 i + 7, the threads' totals meet in a
//                        wave scan and four wave totals), T = the last chunk's cumulative sum, target = u[s] T, the first
//                        chunk with a weight whose cumulative sum exceeds it; that ONE chunk's d2 is scanned again in ascending
//                        row order, 64 rows at a time, for the first row with a weight whose cumulative sum exceeds the target
//                        (two orders of summation may disagree in the last bit on whether a row WITHOUT a weight is already
//                        beyond the target: such a row, a duplicate of a centre, is never taken); the row goes to LDS;
//                        workgroup 0 records idx and potential.  Body: d2 = min(d2, |x - pick|^2) over the own chunk (assigned
//                        in launch 0), and the chunk's float64 sum of weights.
//   kp_finish_kernel     one workgroup, the prologue alone: the last pick
// What the redundant prologue costs: every workgroup reads all per-chunk sums (8 bytes x at most 2,048 = 16 KB from L2, against
// the c x D x 4 bytes of its own chunk: 53 KB at 200,000 x 128, where the sums add 30 % to the bytes requested, all of them L2
// hits) and one chunk's d2 (c x 4 bytes, 416 at that size), then four barriers; batch.hip's prologue reads the same 16 KB of
// (score, index) partials.  It buys the absence of any inter-workgroup wait.  Measured (one MI355X, k = 1,024):
// 29.6 us per pick at 200,000 x 128, 43.7 us at 200,000 pairs x 512 in the pair form — 0.86x / 0.89x batch.hip's pick on the same
// rows, and within 2-3 % of batch.hip with its score's square root and division taken out: the prologue does not show.
//
// Two hazards, both met by double-buffering on the parity of the launch: launch s reads the sums AND d2 of buffer (s - 1) & 1
// and writes buffer s & 1.  The sums as batch.hip's partials.  d2 too, because every workgroup's prologue scans the winning
// chunk while that chunk's owner rewrites it in the same launch: with one buffer a late workgroup could see distances that
// already hold the pick being resolved, and stage a later row than the workgroup that recorded idx.
//
// Every float64 sum runs in an order fixed by (N, D) alone: results are bit-identical from run to run.
#include "batch_rows.h"

namespace alink {
namespace {

constexpr int KP_MAX_GRID = 2048;          // chunks = workgroups of a launch (eight per CU, all resident) = sums every prologue reads
constexpr int KP_PASS_ROWS = 2;            // neighbouring rows per wave and pass
constexpr int KP_WG_PASS = 4 * KP_PASS_ROWS;   // rows a workgroup takes per pass
constexpr int KP_PER_THREAD = KP_MAX_GRID / 256;  // chunk sums per thread of the prologue
constexpr int KP_NONE = 0x7fffffff;
constexpr int KP_TAIL_BYTES = 128;         // the prologue's LDS words, behind the picked row in the dynamic region

struct KpCand { float v; int i; };         // (norm, index): larger wins, equal -> the lower index; a NaN never enters
__device__ __forceinline__ KpCand kp_better(KpCand a, KpCand b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ KpCand kp_wave_max(KpCand a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        KpCand b;
        b.v = __shfl_xor(a.v, o, 64);
        b.i = __shfl_xor(a.i, o, 64);
        a = kp_better(a, b);
    }
    return a;
}
// inclusive scan over the wave's 64 lanes, lane order ascending (Hillis-Steele: distances 1, 2, ..., 32)
__device__ __forceinline__ double kp_wave_scan(double x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}
__device__ __forceinline__ double kp_weight(float d) { return (d > 0.f && d < INFINITY) ? (double)d : 0.0; }

__host__ __device__ __forceinline__ long long kp_chunk_rows(long long N) {
    const long long per = (long long)KP_MAX_GRID * KP_WG_PASS;
    return KP_WG_PASS * ((N + per - 1) / per);
}

// the prologue's LDS words
struct KpShared {
    double wave_total[4];
    double T;
    double base;
    int lo[4];
    int hi[4];
    KpCand cand[4];
};
static_assert(sizeof(KpShared) <= KP_TAIL_BYTES, "KP_TAIL_BYTES");

struct KpPick { long long row; double T; };

// Pick s >= 1 from the per-chunk sums and the d2 of the previous launch; every thread of the workgroup returns the same.
__device__ __forceinline__ KpPick kp_sample(const double* __restrict__ sums, int nchunks, long long chunk, long long N,
                                            const float* __restrict__ d2, double u, KpShared* sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double v[KP_PER_THREAD];
    double mine = 0.0;
#pragma unroll
    for (int j = 0; j < KP_PER_THREAD; ++j) {
        const int c = tid * KP_PER_THREAD + j;
        v[j] = c < nchunks ? sums[c] : 0.0;
        mine += v[j];
    }
    const double incl = kp_wave_scan(mine, lane);
    double before = __shfl_up(incl, 1, 64);               // the lanes below this one, in the wave
    if (lane == 0) before = 0.0;
    if (lane == 63) sh->wave_total[wave] = incl;
    __syncthreads();
    double wbase = 0.0;
    for (int w = 0; w < wave; ++w) wbase += sh->wave_total[w];
    // cumulative sum at the end of each of this thread's chunks: from the sum of everything below, one chunk after another
    double cum[KP_PER_THREAD];
    double c0 = wbase + before;
#pragma unroll
    for (int j = 0; j < KP_PER_THREAD; ++j) {
        c0 += v[j];
        cum[j] = c0;
        if (tid * KP_PER_THREAD + j == nchunks - 1) sh->T = c0;
    }
    __syncthreads();
    KpPick out;
    out.T = sh->T;
    out.row = -1;
    if (!(out.T > 0.0)) return out;                        // fewer distinct rows than picks (uniform over the workgroup)
    const double target = u * out.T;
    int lo = KP_NONE, hi = -1;                             // first chunk with a weight whose cumulative sum exceeds the target; last chunk with a weight
#pragma unroll
    for (int j = KP_PER_THREAD - 1; j >= 0; --j) {
        const int c = tid * KP_PER_THREAD + j;
        if (c < nchunks && v[j] > 0.0 && cum[j] > target) lo = c;
        if (hi < 0 && c < nchunks && v[j] > 0.0) hi = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) { sh->lo[wave] = lo; sh->hi[wave] = hi; }
    __syncthreads();
    lo = min(min(sh->lo[0], sh->lo[1]), min(sh->lo[2], sh->lo[3]));
    hi = max(max(sh->hi[0], sh->hi[1]), max(sh->hi[2], sh->hi[3]));
    const int g = lo != KP_NONE ? lo : hi;                 // no chunk beyond the target (the product rounded up to T): the last with a weight
    if (g < 0) return out;                                 // (T > 0 without a positive chunk: an infinite or NaN sum)
#pragma unroll
    for (int j = 0; j < KP_PER_THREAD; ++j)
        if (tid * KP_PER_THREAD + j == g) sh->base = j == 0 ? wbase + before : cum[j > 0 ? j - 1 : 0];
    __syncthreads();
    // chunk g again, in ascending row order, 64 rows at a time (every wave the same: no further barrier)
    double base = sh->base;
    const long long r0 = (long long)g * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
    long long last = -1;
    for (long long r = r0; r < r1; r += 64) {
        const long long n = r + lane;
        const double w = n < r1 ? kp_weight(d2[n]) : 0.0;
        const double x = kp_wave_scan(w, lane);
        const unsigned long long over = __ballot(w > 0.0 && base + x > target);
        if (over) {
            out.row = r + (__ffsll((long long)over) - 1);
            return out;
        }
        const unsigned long long pos = __ballot(w > 0.0);
        if (pos) last = r + (63 - __clzll((long long)pos));
        base += __shfl(x, 63, 64);
    }
    out.row = last;                                        // the scan's order fell short of the chunk's own sum: the last row with a weight
    return out;
}

// the workgroup's 256 threads reduce the norm kernel's candidates; every thread returns the winner
__device__ __forceinline__ KpCand kp_reduce_cands(const KpCand* __restrict__ cands, int n, KpShared* sh) {
    KpCand c{-INFINITY, KP_NONE};
    for (int i = threadIdx.x; i < n; i += 256) c = kp_better(c, cands[i]);
    c = kp_wave_max(c);
    if ((threadIdx.x & 63) == 0) sh->cand[threadIdx.x >> 6] = c;
    __syncthreads();
    c = sh->cand[0];
    for (int w = 1; w < 4; ++w) c = kp_better(c, sh->cand[w]);
    return c;
}

// pick `step` and its potential, by every thread of the workgroup
__device__ __forceinline__ KpPick kp_resolve(int step, long long first, const KpCand* __restrict__ cands, const double* __restrict__ prev_sums,
                                             const float* __restrict__ prev_d2, const double* __restrict__ uniform, int nchunks,
                                             long long chunk, long long N, KpShared* sh) {
    if (step > 0) return kp_sample(prev_sums, nchunks, chunk, N, prev_d2, uniform[step], sh);
    KpPick p;
    p.T = __builtin_nan("");
    p.row = first;
    if (first < 0) {
        const KpCand c = kp_reduce_cands(cands, nchunks, sh);
        p.row = c.i != KP_NONE ? c.i : -1;
    }
    return p;
}

template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256) void kp_norm_kernel(const RbRows t, long long N, long long chunk, KpCand* __restrict__ cands) {
    __shared__ KpCand s_best[4];
    constexpr int NR = KP_PASS_ROWS;
    const int D = t.D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    KpCand best{-INFINITY, KP_NONE};
    for (long long n0 = r0 + wave * NR; n0 < r1; n0 += KP_WG_PASS) {
        RbRow r[NR];
        float s[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            r[j] = rb_row<PAIR>(t, n0 + j < r1 ? n0 + j : n0);   // past the chunk's end: row n0 again, that result dropped
            s[j] = 0.f;
        }
        for (int e0 = 4 * lane; e0 < D; e0 += 256) {
#pragma unroll
            for (int j = 0; j < NR; ++j) s[j] = rb_acc(s[j], rb_quad<PAIR, VEC>(r[j], e0, D), zero);
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const float sj = rb_wave_sum(s[j]);
            if (n0 + j < r1) best = kp_better(best, KpCand{sj, (int)(n0 + j)});
        }
    }
    if (lane == 0) s_best[wave] = best;                    // (every lane of a wave holds the same candidate)
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = kp_better(best, s_best[w]);
        cands[blockIdx.x] = best;
    }
}

template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256) void kp_step_kernel(const RbRows t, long long N, long long chunk, int step, long long first,
                                                      const KpCand* __restrict__ cands, const double* __restrict__ uniform,
                                                      const float* __restrict__ d2_in, float* __restrict__ d2_out,
                                                      const double* __restrict__ sums_in, double* __restrict__ sums_out,
                                                      int32_t* __restrict__ idx_out, double* __restrict__ potential_out) {
    extern __shared__ __attribute__((aligned(16))) float4 kp_dynamic_lds[];   // the picked row (D up to a multiple of 4), then KpShared
    float* prow = (float*)kp_dynamic_lds;
    constexpr int NR = KP_PASS_ROWS;
    const int D = t.D, Dp = (D + 3) & ~3;
    KpShared* sh = (KpShared*)(prow + Dp);
    double* s_sum = sh->wave_total;                        // (free again once the prologue is over)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const KpPick pk = kp_resolve(step, first, cands, sums_in, d2_in, uniform, (int)gridDim.x, chunk, N, sh);
    const long long pick = pk.row;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        idx_out[step] = (int32_t)pick;
        potential_out[step] = pick < 0 && step > 0 ? 0.0 : pk.T;
    }
    if (pick >= 0) {
        const RbRow src = rb_row<PAIR>(t, pick);
        for (int e = threadIdx.x; e < Dp; e += 256) prow[e] = e < D ? rb_elem<PAIR>(src, e) : 0.f;
    }
    __syncthreads();                                       // the row is staged, and the prologue's words are read
    const long long r0 = (long long)blockIdx.x * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
    double wsum = 0.0;                                     // this wave's rows, in ascending order
    for (long long n0 = r0 + wave * NR; n0 < r1; n0 += KP_WG_PASS) {
        long long n[NR];
        float d[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            n[j] = n0 + j < r1 ? n0 + j : n0;              // past the chunk's end: row n0 again, that result dropped
            d[j] = step > 0 ? d2_in[n[j]] : 0.f;           // no pick at all (nothing but NaN norms): every distance 0, the pool exhausted
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
                d[j] = step > 0 ? fminf(d[j], sj) : sj;
            }
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (n0 + j < r1) {
                if (lane == 0) d2_out[n[j]] = d[j];
                wsum += kp_weight(d[j]);
            }
        }
    }
    if (lane == 0) s_sum[wave] = wsum;                     // (every lane of a wave holds the same sum)
    __syncthreads();
    if (threadIdx.x == 0) sums_out[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
}

__global__ __launch_bounds__(256) void kp_finish_kernel(long long N, long long chunk, int nchunks, int step, long long first,
                                                        const KpCand* __restrict__ cands, const double* __restrict__ uniform,
                                                        const float* __restrict__ d2_in, const double* __restrict__ sums_in,
                                                        int32_t* __restrict__ idx_out, double* __restrict__ potential_out) {
    __shared__ KpShared sh;
    const KpPick pk = kp_resolve(step, first, cands, sums_in, d2_in, uniform, nchunks, chunk, N, &sh);
    if (threadIdx.x == 0) {
        idx_out[step] = (int32_t)pk.row;
        potential_out[step] = pk.row < 0 && step > 0 ? 0.0 : pk.T;
    }
}

size_t kp_d2_bytes(int64_t N) { return ((size_t)N * 4 + 255) & ~(size_t)255; }

template <bool PAIR, bool VEC>
void kp_enqueue(const RbRows& t, long long N, const double* uniform, long long first, int k, int32_t* idx, double* potential,
                char* scratch, hipStream_t st) {
    float* d2[2] = {(float*)scratch, (float*)(scratch + kp_d2_bytes(N))};
    double* sums = (double*)(scratch + 2 * kp_d2_bytes(N));
    KpCand* cands = (KpCand*)(sums + 2 * KP_MAX_GRID);
    const long long chunk = kp_chunk_rows(N);
    const unsigned grid = (unsigned)((N + chunk - 1) / chunk);             // <= KP_MAX_GRID
    const size_t lds = (size_t)((t.D + 3) & ~3) * 4 + KP_TAIL_BYTES;
    if (first < 0) hipLaunchKernelGGL((kp_norm_kernel<PAIR, VEC>), dim3(grid), dim3(256), 0, st, t, N, chunk, cands);
    for (int s = 0; s + 1 < k; ++s)
        hipLaunchKernelGGL((kp_step_kernel<PAIR, VEC>), dim3(grid), dim3(256), lds, st, t, N, chunk, s, first, cands, uniform,
                           d2[(s + 1) & 1], d2[s & 1], sums + (size_t)((s + 1) & 1) * KP_MAX_GRID, sums + (size_t)(s & 1) * KP_MAX_GRID, idx,
                           potential);
    hipLaunchKernelGGL(kp_finish_kernel, dim3(1), dim3(256), 0, st, N, chunk, (int)grid, k - 1, first, cands, uniform, d2[k & 1],
                       sums + (size_t)(k & 1) * KP_MAX_GRID, idx, potential);
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

size_t alink_kmeanspp_scratch_bytes(int64_t N, int k) {
    if (N <= 0 || k <= 0) return 0;
    return 2 * kp_d2_bytes(N) + 2 * (size_t)KP_MAX_GRID * sizeof(double) + (size_t)KP_MAX_GRID * sizeof(KpCand);
}

int alink_kmeanspp(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                   const double* dev_uniform, int64_t first, int k, int32_t* dev_idx, double* dev_potential, void* dev_scratch,
                   void* stream) {
    ALINK_REQUIRE(dev_x && dev_uniform && dev_idx && dev_potential && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_li || (dev_r && dev_ri), ALINK_EINVAL, "the pair form needs dev_r and dev_ri beside dev_li");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d (the picked row is held in LDS)", D, RB_MAX_D);
    ALINK_REQUIRE(k >= 1, ALINK_EINVAL, "k=%d must be >= 1", k);
    ALINK_REQUIRE(first >= -1 && first < N, ALINK_EINVAL, "first=%lld outside -1..N-1 (-1: the row of largest norm)", (long long)first);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    if ((int64_t)k > N) k = (int)N;
    DeviceGuard dg(device_of_pointer(dev_x));
    RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    hipStream_t st = (hipStream_t)stream;
    const bool pair = dev_li != nullptr;
    const bool vec = D % 4 == 0 && (((uintptr_t)dev_x | (pair ? (uintptr_t)dev_r : 0)) & 15) == 0;
    if (pair) {
        if (vec) kp_enqueue<true, true>(t, N, dev_uniform, first, k, dev_idx, dev_potential, (char*)dev_scratch, st);
        else kp_enqueue<true, false>(t, N, dev_uniform, first, k, dev_idx, dev_potential, (char*)dev_scratch, st);
    } else {
        if (vec) kp_enqueue<false, true>(t, N, dev_uniform, first, k, dev_idx, dev_potential, (char*)dev_scratch, st);
        else kp_enqueue<false, false>(t, N, dev_uniform, first, k, dev_idx, dev_potential, (char*)dev_scratch, st);
    }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
