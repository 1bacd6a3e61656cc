// conv_device.h — the device helpers every matrix-core convolution kernel of this library is built from (gfx950).
// One copy: the kernels differ in how they tile and stage, not in these.  Everything sits in an unnamed namespace inside
// alink, as the kernels themselves do.
#pragma once
#include "alink_common.h"

namespace alink {
namespace {

// eight T as one 16-byte vector: an MFMA operand, a ds_read_b128, a global_load_dwordx4
template <typename T> struct Vec8;
template <> struct Vec8<__bf16>   { typedef bf16x8 type; };
template <> struct Vec8<_Float16> { typedef f16x8 type; };

// v_mfma_f32_16x16x32_{bf16,f16}: c += a (16 rows x 32 k) * b (32 k x 16 columns); lane l holds k = 8 (l >> 4) .. + 7 of
// row / column l & 15 of a / b and rows 4 (l >> 4) .. + 3 of column l & 15 of c
template <typename T>
__device__ __forceinline__ f32x4 mfma16(typename Vec8<T>::type a, typename Vec8<T>::type b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 mfma16<__bf16>(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma16<_Float16>(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// 16 bytes per lane, global -> LDS, no VGPR destination.  `lds_wave_base` must be wave-uniform:
// lane l lands at lds_wave_base + 16*l.
__device__ __forceinline__ void dma16(const void* gsrc, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)gsrc,
        (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Bijective XCD-aware remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"): blocks
// with equal blockIdx % 8 share an XCD; give each such group one contiguous range of logical ids.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}

// pixel (0..15) inside a 16-pixel MFMA tile handled by MFMA column lr: even pixels on columns {0-3, 12-15}, odd ones on
// {4-11}, so that with the XOR swizzle chunk ^ ((pos >> 1) & 7) every ds_read_b128 lane group hits 16 distinct 16-byte
// slots for any tap shift (conv3x3_direct.hip)
__device__ __forceinline__ int delta(int lr) { return lr < 4 ? 2 * lr : (lr < 12 ? 2 * (lr - 4) + 1 : 2 * (lr - 8)); }

// Counted wait, then the workgroup barrier: all but the N youngest vector-memory operations of this wave have completed
// (vmcnt: its LDS-DMAs have landed; N = 0 waits for everything, N > 0 leaves in flight what the call site says) AND its own
// LDS reads have returned (lgkmcnt) before it arrives at the barrier.  One asm statement with a memory clobber: no LDS
// access moves across it and hipcc adds no vmcnt(0) of its own (cdna_hip_programming.md §5 "Pipelining across barriers").
// The second wait is not optional: the MFMAs that consume a step's last fragments carry no memory dependence, so the
// compiler sinks them — and the lgkmcnt wait they imply — BELOW this statement; a wave then reaches the barrier with
// ds_reads still queued, a faster wave passes the barrier and issues the DMA that re-fills the buffer those reads are aimed
// at, and the reads return the NEXT tile's bytes.  Seen as rare wrong 224-pixel groups under multi-stream load (round 3:
// 1 row in 10^4 in the 128-channel forms of conv3x3_linear.hip, percent-level in the register-rich 64-channel forms, where
// the compiler hoists eight reads across); single-stream runs never showed it.
template <int N>
__device__ __forceinline__ void wait_then_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

}  // namespace
}  // namespace alink
