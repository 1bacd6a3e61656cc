// head_handle.h — the pair head's handle and the constants of its MFMA forward (head.hip), shared with the kernels that run on
// the same handle from other files (egl.hip, alfamix.hip): the packed weight copies, the LDS image of a 32-pair tile, how large it is,
// and the row norms read off it.
#pragma once
#include "alink_common.h"
#include "net_host.h"

#include <vector>

struct alink_head {
    int device = -1;             // the device the handle's memory lives on (current at create)
    int D, h1, h2;
    int od = 2;                  // outputs: 2 = Dense(2)+softmax (code/siamese.py:31-32), 1 = Dense(1, sigmoid) (code/siamese3.py:25)
    float lr, rho, eps;
    size_t nparams;
    size_t oW1, ob1, oW2, ob2, oW3, ob3;
    float* d_params = nullptr;   // Keras layout: kernel (in,out) row-major, bias; per layer
    float* d_grads = nullptr;
    float* d_acc = nullptr;      // Adadelta accumulators
    float* d_dacc = nullptr;     // Adadelta delta accumulators
    float* d_w1p = nullptr;      // W1 packed for the MFMA forward: [D/8][h1][2][4]
    float* d_w2p = nullptr;      // W2 packed: [h1/8][h2][2][4]
    float* d_w2tp = nullptr;     // W2^T packed: [h2/8][h1][2][4] — the back-projection of egl.hip; allocated by its first call, then
                                 // re-derived with the other packed copies
    float* d_w1tp = nullptr;     // W1^T packed: [h1/8][D][2][4] — the back-projection to the input of alfamix.hip; allocated by its
                                 // first call, then re-derived with the other packed copies
    bool packed_dirty = true;
    // bf16 compute mode (alink_head_set_compute_dtype; BASELINE configs[4] "bf16 fine-tune", mixed precision):
    // master parameters, gradients and Adadelta state stay f32; the forward / backward GEMM operands are bf16 —
    // weights from d_pq (2-byte copy of the flat parameter vector, kept current by the update kernels of the
    // batch<=32 step, else re-quantised lazily), activations and activation gradients rounded to bf16 where they are
    // produced; products are exact in f32 and accumulate in f32.  d_pqf holds the same bf16 values widened to f32 for
    // the large-batch chain and the MFMA predict kernel (a derived cache like d_w1p / d_w2p).  Biases are not quantised.
    int qmode = 0;
    __bf16* d_pq = nullptr;
    float* d_pqf = nullptr;
    __bf16* d_wt = nullptr;      // bf16 mode, predict on the bf16 matrix cores: W1^T [h1][D] then W2^T [h2][h1] (re-derived with the packed copies)
    bool pq_dirty = true, pqf_dirty = true;
    // train/eval scratch for up to `cap` rows
    int cap = 4096;
    float *d_dm = nullptr, *d_z1 = nullptr, *d_z2 = nullptr, *d_dz1 = nullptr, *d_dz2 = nullptr,
          *d_dz3 = nullptr, *d_p = nullptr;
    float* d_tiny = nullptr;     // per-row-group partials of the tiny-batch train step
    float* d_mini = nullptr;     // Dense1 partial sums of SmallRes' three-launch step ([D / 32][n][128]); only for that head shape
    unsigned* d_counter = nullptr;   // row groups finished (tiny_eval), 0 between launches
    alink::DeviceAllocs mem;
    // hipGraph cache of the fine-tune step (a launch-bound chain of 8-9 small kernels): one executable
    // graph per distinct (operand pointers, n, grad_scale, apply); replayed while the caller keeps
    // feeding the same buffers (DenseHead stages every batch into persistent tensors for that purpose)
    struct StepGraph {
        const void *L, *R, *y, *sw, *metrics;
        int n, apply;
        float grad_scale, lr;
        hipGraphExec_t exec;
    };
    std::vector<StepGraph> graphs;
    bool use_graph = false;     // measured on MI355X: replay 67.8 us vs 66.2 us of plain launches — the chain is
                                // bound by kernel-to-kernel dependency latency, not by launch cost; kept as an option
    ~alink_head() {
        for (auto& g : graphs) (void)hipGraphExecDestroy(g.exec);
    }
};

namespace alink {

constexpr int TP = 32;          // pairs per workgroup in the MFMA forward
constexpr int ROWP = TP * 8 + 4;  // floats per k8 block in LDS (pad 4: conflict-free b128 writes)
constexpr int KC = 512;         // K chunk staged per pass

inline size_t fwd_lds_bytes(int h1) {
    const size_t a = (size_t)(KC / 8) * ROWP, b = (size_t)(h1 / 8) * ROWP, c = 4 * TP * 64 + TP * 64;
    size_t m = a > b ? a : b;
    if (c > m) m = c;
    return m * sizeof(float);
}

#ifdef __HIPCC__
// Sum of squares of every row of a tile image in the packed A-operand layout (element (row, k) at
// (k >> 3) * ROWP + row * 8 + (k & 1) * 4 + ((k & 7) >> 1)), nk8 blocks of 8 deep.  Thread t works for row t >> 3: it adds the
// blocks (t & 7), (t & 7) + 8, ... in ascending order, a block in ascending k, and the eight shares meet in an xor butterfly
// (1, 2, 4), which leaves the same bits on all eight lanes.  The order depends on nk8 alone, not on the row.
__device__ __forceinline__ float tile_row_sumsq(const float* buf, int nk8) {
    const int row = threadIdx.x >> 3, part = threadIdx.x & 7;
    float s = 0.f;
    for (int k8 = part; k8 < nk8; k8 += 8) {
        const f32x4 e = *(const f32x4*)(buf + k8 * ROWP + row * 8), o = *(const f32x4*)(buf + k8 * ROWP + row * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s = fmaf(e[j], e[j], s);
            s = fmaf(o[j], o[j], s);
        }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    return s;
}
#endif

// brings the packed copies of W1 / W2 (and the derived copies that exist) up to date with the parameters (head.hip)
int head_ensure_packed(alink_head* h, hipStream_t st);

}  // namespace alink
