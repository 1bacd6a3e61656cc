// knn_lists.h — what knn.hip (a pool against itself) and knn_rect.hip (queries against a separate reference set) share beyond the
// tile product of pool_tile.h: a lane's running sorted list of (score, index) in registers — insertion, the select tree that reads
// one of 16 registers, the (score, index) order and the merge of a row's two lanes.  The header comment of knn.hip describes the
// kernel these serve.
#pragma once
#include "pool_tile.h"

namespace alink {
namespace {

constexpr int KN_MAX_K = 32;

// a candidate of a lane's own stream (ascending index) into its sorted list: strict `<`, so it lands behind its equals
template <int KK>
__device__ __forceinline__ void kn_insert(float (&ls)[KK], int (&lj)[KK], float s, int j) {
#pragma unroll
    for (int p = KK - 1; p > 0; --p) {
        const bool up = s < ls[p - 1], here = s < ls[p];
        ls[p] = up ? ls[p - 1] : (here ? s : ls[p]);
        lj[p] = up ? lj[p - 1] : (here ? j : lj[p]);
    }
    const bool first = s < ls[0];
    ls[0] = first ? s : ls[0];
    lj[0] = first ? j : lj[0];
}
// element r (uniform over the wave) of 16 registers, by a tree of selects: no index reaches the array at run time
template <int LO, int CNT>
__device__ __forceinline__ float kn_pick(const float (&v)[16], int r) {
    if constexpr (CNT == 1) {
        return v[LO];
    } else {
        const float lo = kn_pick<LO, CNT / 2>(v, r), hi = kn_pick<LO + CNT / 2, CNT / 2>(v, r);
        return (r & (CNT / 2)) ? hi : lo;
    }
}
__device__ __forceinline__ float kn_pick16(const float (&v)[16], int r) { return kn_pick<0, 16>(v, r); }

// (score, index) order; an empty slot is (+inf, -1), behind every real entry (whose score is below +inf)
__device__ __forceinline__ bool kn_less(float sa, int ja, float sb, int jb) { return sa < sb || (sa == sb && ja < jb); }

// the two sorted lists of a row's two lanes -> the KK least of both, sorted, in both lanes.  min(A[i], B[KK - 1 - i]) over i holds
// the KK least of the union as a bitonic sequence; log2(KK) half-cleaner stages sort it.  Every index is a constant.
template <int KK>
__device__ __forceinline__ void kn_merge_halves(float (&ls)[KK], int (&lj)[KK]) {
    float os[KK];
    int oj[KK];
#pragma unroll
    for (int p = 0; p < KK; ++p) { os[p] = __shfl_xor(ls[KK - 1 - p], 32, 64); oj[p] = __shfl_xor(lj[KK - 1 - p], 32, 64); }
#pragma unroll
    for (int p = 0; p < KK; ++p) {
        const bool take = kn_less(os[p], oj[p], ls[p], lj[p]);
        ls[p] = take ? os[p] : ls[p];
        lj[p] = take ? oj[p] : lj[p];
    }
#pragma unroll
    for (int st = KK / 2; st > 0; st >>= 1) {
#pragma unroll
        for (int p = 0; p < KK; ++p) {
            if ((p & st) == 0) {
                const bool swap = kn_less(ls[p + st], lj[p + st], ls[p], lj[p]);
                const float s0 = ls[p], s1 = ls[p + st];
                const int j0 = lj[p], j1 = lj[p + st];
                ls[p] = swap ? s1 : s0; ls[p + st] = swap ? s0 : s1;
                lj[p] = swap ? j1 : j0; lj[p + st] = swap ? j0 : j1;
            }
        }
    }
}

}  // namespace
}  // namespace alink
