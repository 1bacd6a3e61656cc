// knn_rect.hip — the K nearest rows of a separate reference set for every query row, and the score of Contrastive Active Learning
// over such lists (Margatina, Vernikos, Barrault & Aletras 2021: the mean KL divergence between the predicted probabilities of a
// pool row's nearest labelled rows and its own; a-link_amd/cal.py).  include/alink_hip.h (alink_knn_rect, alink_cal_score) states
// both rules in full.
//
// What bounds it: an (N x D)(D x M) product on the f32 matrix cores whose scores never reach memory — kn_list_kernel (knn.hip)
// with a second operand.  The queries are the rows of pool_tile.h's tile product, the references walk past as its candidates.
//
// Launches of alink_knn_rect, all on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative
// launch, no grid barrier, no atomics, nothing read back):
//   pt_norm_kernel  (pool_tile.h) twice: |q_n|^2 of every query and |c_j|^2 of every reference, one wave per row
//   kr_list_kernel  kn_list_kernel's lists over pt_product (the header comments of knn.hip and pool_tile.h describe both): a
//                   lane's running KK best (8 / 16 / 32) a sorted list in registers, entered through the wave vote and the
//                   unrolled compare-and-shift chain; the two lanes of a row merge at the end.  What differs: the candidate
//                   operand and its norms come from the reference set, and there is neither a group nor a self test — a query
//                   whose own norm is NaN or +inf holds +inf for every score.
//   kr_dist_kernel  the light pass, one wave per query: d2 of the K winners by direct differences in batch_rows.h's order
// alink_cal_score is one launch, one thread per query: float64 throughout, slots and classes in ascending order.
// Measured: DESIGN.md §9.  Not built: splitting the references over workgroups (a handful of queries against a huge gallery keeps
// few workgroups busy), K > 32, groups, a cosine metric, several ranks' pools in one call.
#include "knn_lists.h"

namespace alink {
namespace {

constexpr int CAL_MAX_C = 32;

// Two waves per SIMD as kn_list_kernel has them; the one form that does not fit 256 registers without scratch — KK = 32 on row
// tables read with scalar loads — keeps one wave.
template <int KK, bool PAIR, bool VEC>
__global__ __launch_bounds__(256, (KK == 32 && !PAIR && !VEC) ? 1 : 2) void kr_list_kernel(const RbRows tq, long long N, const RbRows tc, long long M,
                                                      const float* __restrict__ qnorm, const float* __restrict__ cnorm, int K,
                                                      int32_t* __restrict__ idx, int32_t* __restrict__ found) {
    __shared__ float sX[PT_DC * PT_LD];
    __shared__ float sC[PT_DC * PT_LD];
    __shared__ __attribute__((aligned(16))) float sN[PT_TK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const long long n0 = (long long)blockIdx.x * PT_TN;
    const int srow = tid & 127;            // the tile row this thread stages (pool_tile.h)
    const long long xn = n0 + srow;
    const bool xhave = xn < N;

    // this lane's query; one past the set, or with |q|^2 NaN or +inf, has no neighbours
    const long long n = n0 + wave * 32 + l31;
    const bool alive = n < N && qnorm[n] < INFINITY;

    float ls[KK];                          // a score enters by `<` alone: neither NaN nor +inf ever does
    int lj[KK];
#pragma unroll
    for (int p = 0; p < KK; ++p) { ls[p] = INFINITY; lj[p] = -1; }

    for (long long k0 = 0; k0 < M; k0 += PT_TK) {
        const long long left = M - k0;
        const int nblk = left >= PT_TK ? 4 : (int)((left + 31) >> 5);      // MFMA row blocks of this tile that hold a row (uniform)
        const long long cn_ = k0 + srow;
        const bool chave = cn_ < M;
        f32x16 acc[4];
        pt_product<PAIR, VEC, PAIR, VEC>(tq, xn, xhave, tc, cn_, chave, nblk, sX, sC, acc, [&](int i) {
            const long long j = k0 + i;
            sN[i] = j < M ? cnorm[j] : INFINITY;           // a padded reference never enters
        });
        // the tile's scores against the running list: in a lane the references come in ascending order
        const int jbase = (int)(unsigned)k0 + 4 * hh;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < nblk) {
                // the block's 16 scores of this lane, and which of them SOME lane of the wave holds below its KK-th (uniform): only
                // those walk the insertion chain, in ascending order (kn_list_kernel says why that loses nothing)
                float sc[16];
                unsigned marked = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 cn = *(const float4*)(sN + b * 32 + 8 * g + 4 * hh);
                    const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float s = __builtin_fmaf(-2.f, acc[b][4 * g + i], cnv[i]);
                        sc[4 * g + i] = alive ? s : INFINITY;
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
    kn_merge_halves<KK>(ls, lj);           // the two halves of a query meet
    if (hh == 0 && n < N) {
        int32_t* o = idx + (size_t)n * K;
        int f = 0;
#pragma unroll
        for (int p = 0; p < KK; ++p)
            if (p < K) { o[p] = lj[p]; f += lj[p] >= 0; }
        if (found) found[n] = f;
    }
}

// the light pass, one wave per query: d2 of the winners
template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256) void kr_dist_kernel(const RbRows tq, long long N, const RbRows tc, int K,
                                                      const int32_t* __restrict__ idx, float* __restrict__ d2) {
    const int D = tq.D;
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const RbRow r = rb_row<PAIR>(tq, n);
    for (int p = 0; p < K; ++p) {
        const int j = idx[(size_t)n * K + p];
        float d = __builtin_nanf("");
        if (j >= 0) {                                      // (uniform over the wave)
            const RbRow c = rb_row<PAIR>(tc, j);
            float s = 0.f;
            for (int e0 = 4 * lane; e0 < D; e0 += 256) s = rb_acc(s, rb_quad<PAIR, VEC>(r, e0, D), rb_quad<PAIR, VEC>(c, e0, D));
            d = rb_wave_sum(s);
        }
        if (lane == 0) d2[(size_t)n * K + p] = d;
    }
}

// One thread per query.  float64 throughout and no contraction: every product and every sum rounds once, as the host form's do.
__global__ __launch_bounds__(256) void cal_score_kernel(const float* __restrict__ p, const float* __restrict__ q, int C,
                                                        const int32_t* __restrict__ idx, long long N, long long M, int K,
                                                        float* __restrict__ score) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float* pn = p + (size_t)n * C;
    double total = 0.0;
    int f = 0;
    for (int s = 0; s < K; ++s) {
        const long long j = idx[(size_t)n * K + s];
        if (j < 0 || j >= M) continue;                     // an unfilled slot; an index past the references is never read through
        const float* qj = q + (size_t)j * C;
        double kl = 0.0;
        for (int c = 0; c < C; ++c) {
            const double qv = (double)qj[c], pv = (double)pn[c];
            const double pf = pv > 0x1p-126 ? pv : 0x1p-126;
            if (qv > 0.0) kl = kl + qv * (log(qv) - log(pf));
        }
        total = total + kl;
        ++f;
    }
    score[n] = f ? (float)(total / (double)f) : 0.f;
}

struct KrArgs {
    int K;
    int32_t* idx;
    float* d2;
    int32_t* found;
};

template <bool PAIR, bool VEC>
void kr_enqueue(const RbRows& tq, long long N, const RbRows& tc, long long M, const KrArgs& a, float* qnorm, float* cnorm, hipStream_t st) {
    const unsigned qgrid = (unsigned)((N + 3) / 4), cgrid = (unsigned)((M + 3) / 4);
    const unsigned lgrid = (unsigned)((N + PT_TN - 1) / PT_TN);
    hipLaunchKernelGGL((pt_norm_kernel<PAIR, VEC>), dim3(qgrid), dim3(256), 0, st, tq, N, qnorm);
    hipLaunchKernelGGL((pt_norm_kernel<PAIR, VEC>), dim3(cgrid), dim3(256), 0, st, tc, M, cnorm);
    if (a.K <= 8)
        hipLaunchKernelGGL((kr_list_kernel<8, PAIR, VEC>), dim3(lgrid), dim3(256), 0, st, tq, N, tc, M, qnorm, cnorm, a.K, a.idx, a.found);
    else if (a.K <= 16)
        hipLaunchKernelGGL((kr_list_kernel<16, PAIR, VEC>), dim3(lgrid), dim3(256), 0, st, tq, N, tc, M, qnorm, cnorm, a.K, a.idx, a.found);
    else
        hipLaunchKernelGGL((kr_list_kernel<32, PAIR, VEC>), dim3(lgrid), dim3(256), 0, st, tq, N, tc, M, qnorm, cnorm, a.K, a.idx, a.found);
    if (a.d2) hipLaunchKernelGGL((kr_dist_kernel<PAIR, VEC>), dim3(qgrid), dim3(256), 0, st, tq, N, tc, a.K, a.idx, a.d2);
}

bool kr_sizes_ok(int64_t N, int64_t M, int D, int K) {
    return N >= 1 && N < (1ll << 31) && M >= 1 && M < (1ll << 31) && D >= 1 && D <= RB_MAX_D && K >= 1 && K <= KN_MAX_K;
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

size_t alink_knn_rect_scratch_bytes(int64_t N, int64_t M, int D, int K) {
    if (!kr_sizes_ok(N, M, D, K)) return 0;
    return pt_align((size_t)N * 4) + pt_align((size_t)M * 4);
}

int alink_knn_rect(const float* dev_qx, const float* dev_qr, const int32_t* dev_qli, const int32_t* dev_qri, int64_t N,
                   const float* dev_cx, const float* dev_cr, const int32_t* dev_cli, const int32_t* dev_cri, int64_t M, int D, int K,
                   int32_t* dev_idx, float* dev_d2, int32_t* dev_found, void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_qx && dev_cx && dev_idx && dev_scratch, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_qli || (dev_qr && dev_qri), ALINK_EINVAL, "the pair form needs dev_qr and dev_qri beside dev_qli");
    ALINK_REQUIRE(!dev_cli || (dev_cr && dev_cri), ALINK_EINVAL, "the pair form needs dev_cr and dev_cri beside dev_cli");
    ALINK_REQUIRE((dev_qli != nullptr) == (dev_cli != nullptr), ALINK_EINVAL,
                  "mixed forms: queries and references are both row tables or both pair forms (materialise the smaller side)");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(M >= 1 && M < (1ll << 31), ALINK_EINVAL, "M=%lld outside 1..2^31-1", (long long)M);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d", D, RB_MAX_D);
    ALINK_REQUIRE(K >= 1 && K <= KN_MAX_K, ALINK_EINVAL, "K=%d outside 1..%d", K, KN_MAX_K);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_qx));
    const RbRows tq{dev_qx, dev_qr, dev_qli, dev_qri, D}, tc{dev_cx, dev_cr, dev_cli, dev_cri, D};
    const KrArgs a{K, dev_idx, dev_d2, dev_found};
    hipStream_t st = (hipStream_t)stream;
    const bool pair = dev_qli != nullptr;
    const bool vec = pt_vec(tq) && pt_vec(tc);
    float* qnorm = (float*)dev_scratch;
    float* cnorm = (float*)((char*)dev_scratch + pt_align((size_t)N * 4));
    if (pair) { if (vec) kr_enqueue<true, true>(tq, N, tc, M, a, qnorm, cnorm, st); else kr_enqueue<true, false>(tq, N, tc, M, a, qnorm, cnorm, st); }
    else { if (vec) kr_enqueue<false, true>(tq, N, tc, M, a, qnorm, cnorm, st); else kr_enqueue<false, false>(tq, N, tc, M, a, qnorm, cnorm, st); }
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

int alink_cal_score(const float* dev_p, const float* dev_q, int C, const int32_t* dev_idx, int64_t N, int64_t M, int K,
                    float* dev_score, void* stream) {
    ALINK_REQUIRE(dev_p && dev_q && dev_idx && dev_score, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(M >= 1 && M < (1ll << 31), ALINK_EINVAL, "M=%lld outside 1..2^31-1", (long long)M);
    ALINK_REQUIRE(K >= 1 && K <= KN_MAX_K, ALINK_EINVAL, "K=%d outside 1..%d", K, KN_MAX_K);
    ALINK_REQUIRE(C >= 1 && C <= CAL_MAX_C, ALINK_EINVAL, "C=%d outside 1..%d", C, CAL_MAX_C);
    DeviceGuard dg(device_of_pointer(dev_p));
    hipLaunchKernelGGL(cal_score_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dev_p, dev_q, C, dev_idx,
                       (long long)N, (long long)M, K, dev_score);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
