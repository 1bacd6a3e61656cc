// conv_kernel.h — the convolution kernels by name, the facts callers ask about each, and the one statement of where a
// folded weight sits in the buffer a kernel reads.  Host-side, plain C++ (no HIP, no device code): the layout can be
// compiled and exercised with the host compiler alone.
#pragma once
#include <stddef.h>

namespace alink {

// Which kernel runs a convolution.  Chosen once per layer when its weights are packed (direct_variant,
// direct_variant_tiles, linear_variant_x2 in alink_common.h) and handed to launch_conv.  The values are the variant numbers
// the records under profiles/ cite.
enum class ConvKernel : int {
    Igemm = 0,          // conv_igemm.hip: any kernel size and stride — also the answer when no 3x3 kernel below applies
    // conv3x3_direct.hip, row-aligned tiles, 8 waves, one workgroup per CU (D1..D6): map width, Cout a multiple of
    TileW14C256 = 1,
    TileW28C256 = 2,
    TileW28C128 = 3,
    TileW56C128 = 4,
    TileW56C64 = 5,
    TileW112C64 = 6,
    // conv3x3_direct.hip, 4 waves and a single input buffer, two workgroups per CU (S1, S3)
    PairW14C128 = 7,
    PairW28C128 = 8,
    // conv3x3_linear.hip, 224-pixel linear tiles, by the width of the (square) map
    Linear14 = 11,
    Linear28 = 12,
    Linear56 = 13,
    Linear7 = 14,
    Linear112 = 15,     // split precision only
    // rolling-row kernels with the weights in registers (64 -> 64 channels at 112 x 112)
    Roll112 = 21,       // conv3x3_c64.hip: stride 1
    Roll112S2 = 25,     // conv3x3_s2c64.hip: stride 2, optionally with the unit's projection shortcut as extra K-steps
};

enum class SplitUnit { None, Chunk, KStep };

struct ConvKernelTraits {
    int       row_perm;        // permutation of the weight rows it reads (permuted_row): 16 = perm64, 17 = perm64b, 8 = perm32
    bool      chunk_major;     // K order of a weight row: [ci / 64][tap][ci % 64]; else tap-major [tap][ci]
    int       channel_block;   // linear tiles: output channels per workgroup (0: not a linear-tile kernel)
    bool      fine;            // linear tiles: has the 64-channel form of the same sums (ConvParams::fine)
    SplitUnit split;           // what a K split over workgroup rows divides: 64-channel input chunks of nine K-steps, single
                               // K-steps, or nothing (the kernel has no split form)
};

inline ConvKernelTraits traits(ConvKernel k) {
    switch (k) {
        case ConvKernel::Igemm:       return {16, false, 0, false, SplitUnit::KStep};
        case ConvKernel::TileW14C256:
        case ConvKernel::TileW28C256:
        case ConvKernel::PairW14C128:
        case ConvKernel::PairW28C128: return {17, true, 0, false, SplitUnit::None};      // 4 MFMA tiles of channels per wave
        case ConvKernel::TileW28C128:
        case ConvKernel::TileW56C128:
        case ConvKernel::TileW56C64:
        case ConvKernel::TileW112C64: return {8, true, 0, false, SplitUnit::None};       // 2 per wave
        case ConvKernel::Linear14:
        case ConvKernel::Linear28:
        case ConvKernel::Linear7:     return {17, true, 128, true, SplitUnit::Chunk};
        case ConvKernel::Linear56:
        case ConvKernel::Linear112:   return {8, true, 64, false, SplitUnit::Chunk};
        case ConvKernel::Roll112:
        case ConvKernel::Roll112S2:   return {8, true, 0, false, SplitUnit::None};
    }
    return {16, false, 0, false, SplitUnit::None};
}

// workgroups of a linear-tile launch: 224 pixels x channel_block output channels each
inline long long linear_grid(long long M, int Cout, int channel_block) { return (M + 223) / 224 * (Cout / channel_block); }

// ---- weight rows ------------------------------------------------------------------------------------------------------
// position of natural channel c (0..63 within its 64-block) in the permuted weight rows
static inline int perm64_row_of_channel(int c) {
    // MFMA tile t (0..3), row 4q+j  <->  channel 16q + 4t + j
    int q = c >> 4, t = (c >> 2) & 3, j = c & 3;
    return 16 * t + 4 * q + j;
}
// same for kernels whose waves own 32 channels (2 MFMA tiles): tile t (0..1), row 4q+j <-> 8q + 4t + j
static inline int perm32_row_of_channel(int c) {
    int q = c >> 3, t = (c >> 2) & 1, j = c & 3;
    return 16 * t + 4 * q + j;
}
// conv3x3_direct with 4 MFMA tiles per wave: tile t = 2 th + tl, row 4q+j  <->  channel 32 th + 8q + 4 tl + j,
// i.e. a lane holds two runs of 8 consecutive channels, 32 apart
static inline int perm64b_row_of_channel(int c) {
    int th = c >> 5, q = (c >> 3) & 3, tl = (c >> 2) & 1, j = c & 3;
    return 16 * (2 * th + tl) + 4 * q + j;
}
// weight row of output channel co; cpl: 16 = perm64 (conv_igemm, stems), 17 = perm64b, 8 = perm32
static inline int permuted_row(int co, int cpl) {
    if (cpl == 17) return (co & ~63) + perm64b_row_of_channel(co & 63);
    return cpl == 16 ? (co & ~63) + perm64_row_of_channel(co & 63) : (co & ~31) + perm32_row_of_channel(co & 31);
}

// ---- packed weight layout -----------------------------------------------------------------------------------------------
// Where the folded weight (output row, tap, input channel) of a convolution sits in the buffer kernel `k` reads.  A buffer is
// `rows` rows of row_pitch() elements, the rows permuted per 64- or 32-block (permuted_row); inside a row
//   16-bit:           tap-major [tap][ci]                        chunk-major [ci / 64][tap][ci % 64]
//                     then cin2 columns of a fused 1x1 projection shortcut behind the taps (row pitch taps * cin + cin2)
//   split precision:  tap-major [tap][ci / 64][hi 64 | lo 64]    chunk-major [ci / 64][hi: taps x 64 | lo: taps x 64]
//                     (ALINK_DT_F16X2: every value an f16 pair; at() is the hi half, the lo half lo_offset() further on)
// The weights of a backward (input-gradient) convolution are the same layout with the roles of Cin and Cout exchanged:
// rows = the forward Cin, cin = the forward Cout.  (The stems' 27- and 147-column rows and the FC layer are packed where
// they are built; they are not convolutions of this family.)
struct WeightLayout {
    int  row_perm;
    bool chunk_major, split;
    int  taps, cin, cin2;

    size_t row_pitch() const { return split ? (size_t)2 * taps * cin : (size_t)taps * cin + cin2; }
    size_t size(int rows) const { return (size_t)rows * row_pitch(); }
    size_t at(int row, int tap, int ci) const {
        const size_t r = (size_t)permuted_row(row, row_perm) * row_pitch(), cc = (size_t)(ci >> 6), j = (size_t)(ci & 63);
        if (split) return r + (chunk_major ? (cc * 2 * taps + tap) * 64 + j : (((size_t)tap * (cin >> 6) + cc) * 2) * 64 + j);
        return r + (chunk_major ? (cc * taps + tap) * 64 + j : (size_t)tap * cin + ci);
    }
    size_t lo_offset() const { return chunk_major ? (size_t)taps * 64 : 64; }
    size_t at_shortcut(int row, int ci2) const { return (size_t)permuted_row(row, row_perm) * row_pitch() + (size_t)taps * cin + ci2; }
};

inline WeightLayout weight_layout(ConvKernel k, int ksz, int cin, bool split = false, int cin2 = 0) {
    const ConvKernelTraits t = traits(k);
    return {t.row_perm, t.chunk_major, split, ksz * ksz, cin, cin2};
}

}  // namespace alink
