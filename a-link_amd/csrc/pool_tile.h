// pool_tile.h — the one tile product behind km_assign_kernel (kmeans.hip), kn_list_kernel (knn.hip), kr_list_kernel (knn_rect.hip)
// and pb_tile_kernel (probcover.hip): 128 rows of a pool against 128 candidates on the f32 matrix cores, with the norm pass, the
// staging fetch and the small host helpers those files share.
//
// Geometry.  A workgroup of 256 threads (4 waves) owns PT_TN = 128 rows, 32 per wave, and walks the candidates in tiles of
// PT_TK = 128: four MFMA row blocks of 32 per wave.  Both operands go through LDS in chunks of PT_DC = 32 columns, stored
// column-major at pitch PT_LD = 132 floats (column e of the tile at e * PT_LD), so that a wave's lanes write 64 neighbouring floats
// of one column while staging and an MFMA operand read is conflict-free.  Staging: thread -> tile row (tid & 127), column quads
// (tid >> 7) + 2 q, q = 0 .. 3; the pair form takes |l - r| on the way.  MFMA M = candidates, N = rows: lane (l, h) of a wave
// holds in acc[b] for row l of its wave the 16 candidates 8 g + 4 h + i (g, i = 0 .. 3; register 4 g + i) of block b —
// ascending in the register index.
//
// What the callers' correctness rests on.  v_mfma_f32_32x32x2_f32 is bit for bit an ascending fmaf chain (sgemm.hip), so x . c is
// ONE chain over e = 0 .. D - 1 from 0 whatever tile a row or a candidate falls in: the accumulators live across the chunks, and
// an absent row, an absent candidate or a column at or past D is staged as zeros (fma(0, 0, acc) = acc).  The tile's side arrays
// (norms, groups) are written between the two barriers of the FIRST chunk: the first barrier is the one every thread passes only
// after its epilogue reads of the previous tile, the second publishes them with the operands.
#pragma once
#include "batch_rows.h"

namespace alink {
namespace {

constexpr int PT_TN = 128;                 // rows of a workgroup: 32 per wave
constexpr int PT_TK = 128;                 // candidates of a tile: four MFMA row blocks per wave
constexpr int PT_DC = 32;                  // columns of a chunk in LDS
constexpr int PT_LD = PT_TN + 4;           // LDS row pitch (floats): column e of the tile at e * PT_LD
constexpr int PT_SLICE_ALIGN = 256;        // rows a scanning wave takes per step

// |x_n|^2: the squared distance of row n to the zero row in the order of batch_rows.h.  One wave per row.
template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256) void pt_norm_kernel(const RbRows t, long long N, float* __restrict__ xnorm) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const RbRow r = rb_row<PAIR>(t, n);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    for (int e0 = 4 * lane; e0 < t.D; e0 += 256) s = rb_acc(s, rb_quad<PAIR, VEC>(r, e0, t.D), zero);
    s = rb_wave_sum(s);
    if (lane == 0) xnorm[n] = s;
}

// columns e0 .. e0 + 3 of a tile row; absent rows and columns are zeros
template <bool PAIR, bool VEC>
__device__ __forceinline__ float4 pt_fetch(const RbRows& t, long long n, bool have, int e0) {
    if (!have || e0 >= t.D) return make_float4(0.f, 0.f, 0.f, 0.f);
    return rb_quad<PAIR, VEC>(rb_row<PAIR>(t, n), e0, t.D);
}

// acc[b] = the products of this wave's 32 rows with block b of the tile's candidates, b < nblk (uniform; the blocks that hold a
// candidate), over all of D.  (tx, xn, xhave), (tc, cn, chave): the staging thread's row and candidate, each table with a row form
// and a load width of its own.  side(i), i = tid < PT_TK, stages what the caller keeps beside candidate i of the tile.  Called by
// all 256 threads of the workgroup (it holds barriers); what side wrote stays valid until the caller's next call.
template <bool PAIRX, bool VECX, bool PAIRC, bool VECC, class Side>
__device__ __forceinline__ void pt_product(const RbRows& tx, long long xn, bool xhave, const RbRows& tc, long long cn, bool chave, int nblk,
                                           float* sX, float* sC, f32x16 (&acc)[4], Side side) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int srow = tid & 127, sq0 = tid >> 7;
    const int D = tx.D;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
    for (int d0 = 0; d0 < D; d0 += PT_DC) {
        float4 vx[4], vc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e0 = d0 + 4 * (sq0 + 2 * q);
            vx[q] = pt_fetch<PAIRX, VECX>(tx, xn, xhave, e0);
            vc[q] = pt_fetch<PAIRC, VECC>(tc, cn, chave, e0);
        }
        __syncthreads();                                   // the previous chunk's operands (and the previous tile's side arrays) are read
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 4 * (sq0 + 2 * q);
            sX[(c + 0) * PT_LD + srow] = vx[q].x; sX[(c + 1) * PT_LD + srow] = vx[q].y;
            sX[(c + 2) * PT_LD + srow] = vx[q].z; sX[(c + 3) * PT_LD + srow] = vx[q].w;
            sC[(c + 0) * PT_LD + srow] = vc[q].x; sC[(c + 1) * PT_LD + srow] = vc[q].y;
            sC[(c + 2) * PT_LD + srow] = vc[q].z; sC[(c + 3) * PT_LD + srow] = vc[q].w;
        }
        if (d0 == 0 && tid < PT_TK) side(tid);
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float xv[8], cv[4][8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = 16 * half + 2 * i + hh;
                xv[i] = sX[e * PT_LD + wave * 32 + l31];
#pragma unroll
                for (int b = 0; b < 4; ++b) cv[b][i] = sC[e * PT_LD + b * 32 + l31];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (b < nblk) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(cv[b][i], xv[i], acc[b], 0, 0, 0);
            }
        }
    }
}

// slices of a scan over N rows for K clusters or groups: a function of (N, K) alone.  *len = rows of a slice (a multiple of
// 256), -> their number
inline int pt_slices(long long N, int K, long long* len) {
    long long S = K >= 2048 ? 1 : (4096 + K - 1) / K;
    if (S > 64) S = 64;
    long long L = (N + S - 1) / S;
    L = (L + PT_SLICE_ALIGN - 1) / PT_SLICE_ALIGN * PT_SLICE_ALIGN;
    *len = L;
    return (int)((N + L - 1) / L);
}

inline size_t pt_align(size_t b) { return (b + 255) & ~(size_t)255; }

// 16-byte loads: D a multiple of 4 and the table (both tables of the pair form) 16-byte aligned
inline bool pt_vec(const RbRows& t) { return t.D % 4 == 0 && (((uintptr_t)t.x | (t.li ? (uintptr_t)t.r : 0)) & 15) == 0; }

}  // namespace
}  // namespace alink
