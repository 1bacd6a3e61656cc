// density.hip — information density (modAL.density: Settles & Craven 2008) and the ranked batch's cold start (modAL.batch's
// select_cold_start_instance) on device: every pool row against every reference row, vector-ALU work, no MFMA.
//
// The rule (include/alink_hip.h states it in full): for pool row n and the R reference rows z_j, d_nj = sqrt(|x_n - z_j|^2) and
// s_nj = 1 / (1 + d_nj); density[n] = mean_j s_nj, mean_distance[n] = mean_j d_nj, central = argmin_n sum_j d_nj.  The reference
// rows are a materialised (R, D) table, or the pool itself (self-pairs count: d = 0, s = 1).
//
// Launches, on the caller's stream, whose order is the ONLY ordering between workgroups (no cooperative launch, no grid barrier,
// no atomics):
//   dn_sum_kernel      rb_init_kernel of batch.hip with another epilogue: a workgroup owns 32 pool rows, the reference rows pass
//                      through LDS in tiles, a wave takes 4 pool rows x 4 reference rows at a time and the 16 squared distances
//                      meet in the packed butterfly (batch_rows.h: the summation order of batch.hip, so the same bits).  That
//                      leaves every distance on four lanes, so the wave first collects FOUR blocks (16 reference rows) and lane L
//                      finishes the one pair that is its own — pool row L >> 4 of the four, reference row 4 (L & 3) + ((L >> 2) & 3)
//                      of the sixteen: one sqrt, one division and a float64 addition per sum and row group per lane and 64 pairs.
//   dn_central_kernel  (only when the central row is asked for) one workgroup, the argmin of the float64 distance sums
//
// The order of a row's two float64 sums is a function of (R, D) alone.  Tiles hold T = 8192 / Dp reference rows (Dp = D rounded
// up to a multiple of 4; T rounded down to a multiple of 16 when it is larger than 16) and pass in ascending order; within a
// tile, position p belongs to the group p / 16 and, inside it, to the lane c of the row's sixteen lanes with
// 4 (c & 3) + (c >> 2) == p % 16; a lane adds its pairs in ascending reference order; the sixteen lane sums then meet once, after
// the last tile, in an xor butterfly (8, 4, 2, 1).
#include "batch_rows.h"

namespace alink {
namespace {

constexpr int DN_NONE = 0x7fffffff;        // index of a candidate that has seen no sum at all

// (sum, index): b replaces a when strictly smaller, or equal with the lower index — a total order, so the minimum does not
// depend on the order the candidates meet in.  A NaN compares false both ways and never enters.
struct DnCand { double v; int i; };
__device__ __forceinline__ DnCand dn_better(DnCand a, DnCand b) { return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// (s, d) with d = sqrt(d2), s = 1 / (1 + d): every operation rounded once, sqrt and division correctly rounded (the compiler's
// default for float)
__device__ __forceinline__ float2 dn_finish_pair(float d2) {
#pragma clang fp contract(off)
    const float d = sqrtf(d2);
    const float s = 1.f / (1.f + d);
    return make_float2(s, d);
}

// SHORT (D <= 512, at most two quads per lane): the four pool rows stay in registers while the whole tile passes; otherwise,
// any D, they are read again for every block.  ref == nullptr: the pool is its own reference, its rows staged as the bits the
// materialised row would hold.
template <bool PAIR, bool VEC, bool SHORT>
__global__ __launch_bounds__(256) void dn_sum_kernel(const RbRows t, long long N, const float* __restrict__ ref, long long R, int tile_rows,
                                                     float* __restrict__ density, float* __restrict__ mean_distance,
                                                     double* __restrict__ distance_sum) {
    __shared__ __attribute__((aligned(16))) float tile[RB_MAX_D];
    constexpr int RW = RB_WG_ROWS / 4, G = RW / 4;
    const int D = t.D, Dp = (D + 3) & ~3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * RB_WG_ROWS + wave * RW;
    const int mine = 4 * (lane & 3) + ((lane >> 2) & 3);   // the reference row of sixteen whose pair this lane finishes
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    double sum_s[G], sum_d[G];                             // lane L: its share of the sums of the wave's row 4 g + (L >> 4)
#pragma unroll
    for (int g = 0; g < G; ++g) sum_s[g] = sum_d[g] = 0.0;
    for (long long m0 = 0; m0 < R; m0 += tile_rows) {
        const int tm = (int)(R - m0 < tile_rows ? R - m0 : tile_rows);
        __syncthreads();                                   // the previous tile has been consumed
        for (int r = wave; r < tm; r += 4) {               // a wave copies a reference row
            if (ref) {
                const float* src = ref + (size_t)(m0 + r) * D;
                for (int c = lane; c < Dp; c += 64) tile[r * Dp + c] = c < D ? src[c] : 0.f;
            } else {
                const RbRow src = rb_row<PAIR>(t, m0 + r);
                for (int c = lane; c < Dp; c += 64) tile[r * Dp + c] = c < D ? rb_elem<PAIR>(src, c) : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
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
            for (int m = 0; m < tm; m += 16) {
                float d2 = 0.f;                            // of this lane's own pair among the 4 x 16
#pragma unroll 1
                for (int j = 0; j < 4 && m + 4 * j < tm; ++j) {
                    const float* z[4];                     // a row past the tile's last is that last row again, its pairs dropped
                    float s[16];
#pragma unroll
                    for (int b = 0; b < 4; ++b) z[b] = tile + (m + 4 * j + b < tm ? m + 4 * j + b : tm - 1) * Dp + 4 * lane;
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[i] = 0.f;
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
                    const float v = rb_block_pair_sums(s, lane);
                    if ((lane & 3) == j) d2 = v;
                }
                if (m + mine < tm) {
                    // g is a loop counter, so the group's sums are chosen by a select, not by an index (an indexed register
                    // array goes to scratch); the other group's sums take + 0.0, which leaves their bits.  Unrolling the loop
                    // over g instead costs 12 to 32 registers and with them the fourth wave per SIMD: 45 ms where this takes 39.
                    const float2 sd = dn_finish_pair(d2);
#pragma unroll
                    for (int h = 0; h < G; ++h) {
                        sum_s[h] += h == g ? (double)sd.x : 0.0;
                        sum_d[h] += h == g ? (double)sd.y : 0.0;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        double ss = sum_s[g], sd = sum_d[g];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            ss += __shfl_xor(ss, o, 64);
            sd += __shfl_xor(sd, o, 64);
        }
        const long long n = row0 + 4 * g + (lane >> 4);
        if ((lane & 15) == 0 && n < N) {
            if (density) density[n] = (float)(ss / (double)R);
            if (mean_distance) mean_distance[n] = (float)(sd / (double)R);
            if (distance_sum) distance_sum[n] = sd;
        }
    }
}

__global__ __launch_bounds__(256) void dn_central_kernel(const double* __restrict__ distance_sum, long long N, int32_t* __restrict__ central) {
    __shared__ DnCand s_w[4];
    DnCand c{(double)INFINITY, DN_NONE};
    for (long long n = threadIdx.x; n < N; n += 256) c = dn_better(c, DnCand{distance_sum[n], (int)n});
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        DnCand b;
        b.v = __shfl_xor(c.v, o, 64);
        b.i = __shfl_xor(c.i, o, 64);
        c = dn_better(c, b);
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) c = dn_better(c, s_w[w]);
        central[0] = c.i != DN_NONE ? c.i : -1;
    }
}

template <bool PAIR, bool VEC>
void dn_enqueue(const RbRows& t, long long N, const float* ref, long long R, float* density, float* mean_distance, double* distance_sum,
                hipStream_t st) {
    const int Dp = (t.D + 3) & ~3;
    int tile_rows = RB_MAX_D / Dp;                         // >= 1: D <= RB_MAX_D; >= 16 for D <= 512
    if (tile_rows > 16) tile_rows &= ~15;                  // whole groups of sixteen
    const unsigned blocks = (unsigned)((N + RB_WG_ROWS - 1) / RB_WG_ROWS);
    if (t.D <= 512) hipLaunchKernelGGL((dn_sum_kernel<PAIR, VEC, true>), dim3(blocks), dim3(256), 0, st, t, N, ref, R, tile_rows, density,
                                       mean_distance, distance_sum);
    else hipLaunchKernelGGL((dn_sum_kernel<PAIR, VEC, false>), dim3(blocks), dim3(256), 0, st, t, N, ref, R, tile_rows, density,
                            mean_distance, distance_sum);
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

size_t alink_information_density_scratch_bytes(int64_t N) {
    if (N <= 0) return 0;
    return ((size_t)N * 8 + 255) & ~(size_t)255;
}

int alink_information_density(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                              const float* dev_ref, int64_t R, float* dev_density, float* dev_mean_distance, int32_t* dev_central,
                              void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_x, ALINK_EINVAL, "NULL argument");
    ALINK_REQUIRE(!dev_li || (dev_r && dev_ri), ALINK_EINVAL, "the pair form needs dev_r and dev_ri beside dev_li");
    ALINK_REQUIRE(N >= 1 && N < (1ll << 31), ALINK_EINVAL, "N=%lld outside 1..2^31-1", (long long)N);
    ALINK_REQUIRE(R >= 1 && R < (1ll << 31), ALINK_EINVAL, "R=%lld outside 1..2^31-1", (long long)R);
    ALINK_REQUIRE(dev_ref || R == N, ALINK_EINVAL, "R=%lld: without dev_ref the pool is its own reference and R must be N=%lld",
                  (long long)R, (long long)N);
    ALINK_REQUIRE(D >= 1 && D <= RB_MAX_D, ALINK_EINVAL, "D=%d outside 1..%d (a reference row is held in LDS)", D, RB_MAX_D);
    ALINK_REQUIRE(dev_density || dev_mean_distance || dev_central, ALINK_EINVAL, "no output: density, mean distance and central row are all NULL");
    ALINK_REQUIRE(!dev_central || (dev_scratch && ((uintptr_t)dev_scratch & 255) == 0), ALINK_EINVAL,
                  "the central row needs scratch, 256-byte aligned");
    DeviceGuard dg(device_of_pointer(dev_x));
    RbRows t{dev_x, dev_r, dev_li, dev_ri, D};
    double* distance_sum = dev_central ? (double*)dev_scratch : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const bool pair = dev_li != nullptr;
    const bool vec = D % 4 == 0 && (((uintptr_t)dev_x | (pair ? (uintptr_t)dev_r : 0)) & 15) == 0;
    if (pair) {
        if (vec) dn_enqueue<true, true>(t, N, dev_ref, R, dev_density, dev_mean_distance, distance_sum, st);
        else dn_enqueue<true, false>(t, N, dev_ref, R, dev_density, dev_mean_distance, distance_sum, st);
    } else {
        if (vec) dn_enqueue<false, true>(t, N, dev_ref, R, dev_density, dev_mean_distance, distance_sum, st);
        else dn_enqueue<false, false>(t, N, dev_ref, R, dev_density, dev_mean_distance, distance_sum, st);
    }
    if (dev_central) hipLaunchKernelGGL(dn_central_kernel, dim3(1), dim3(256), 0, st, distance_sum, N, dev_central);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
