// select.hip — pool scoring and top-k on device (HBM-bound integer/compare work, no MFMA).
//
// Replaces, for large pools, the host NumPy at
//   code/uncertainty.py:15-60   (_proba_uncertainty / _proba_margin / _proba_entropy)
//   code/uncertainty.py:155,183,213 (multi_argmax top-n)   and   code/ALINK_arc.py:170-181
//   (disparity = -|M2[:,c] - M1[:,c]| ; argsort(...)[:int(P*ratio)]).
//
// top-k = exact radix SELECT on unique 64-bit keys (order-preserving score bits << 32 | index, so
// ties break towards the lower index deterministically — the reference's np.argsort/argpartition
// tie order is unspecified), then a bitonic sort of just the k survivors.  Each select pass streams
// the P keys once (8 B/key), histogramming in LDS.
//
// alink_identify_rows replaces the per-probe np.argmax of code/ALINK_MTP.py:285 over a whole (P, G, C) score array: one
// workgroup per probe row, wave reductions, no atomics.
#include "alink_common.h"

namespace alink {
namespace {

struct SelState {
    unsigned long long prefix;   // bits decided so far (high bits), rest zero
    unsigned long long mask;     // mask of decided bits
    unsigned long long krem;     // rank still to find inside the matching set (1-based)
    unsigned int count;          // compaction counter
    unsigned int pad;
    unsigned int hist[256];
};

__device__ __forceinline__ unsigned int ord32(float f) {
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // ascending float order as unsigned
}

__global__ void score_kernel(int kind, const float* __restrict__ a, const float* __restrict__ b, int col,
                             long long P, int C, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float* p = a + i * C;
    float r;
    if (kind == ALINK_SCORE_UNCERTAINTY) {
        float m = p[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
        r = 1.f - m;
    } else if (kind == ALINK_SCORE_MARGIN) {
        if (C == 1) { r = 0.f; }
        else {
            float m1 = -INFINITY, m2 = -INFINITY;
            for (int c = 0; c < C; ++c) {
                const float v = p[c];
                if (v > m1) { m2 = m1; m1 = v; } else if (v > m2) { m2 = v; }
            }
            r = m1 - m2;
        }
    } else if (kind == ALINK_SCORE_ENTROPY) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += p[c];
        float e = 0.f;
        for (int c = 0; c < C; ++c) {
            const float q = p[c] / s;
            e += (q > 0.f) ? -q * logf(q) : 0.f;
        }
        r = e;
    } else {
        r = -fabsf(b[i * C + col] - p[col]);
    }
    out[i] = r;
}

__global__ void make_keys_kernel(const float* __restrict__ s, long long P, int largest,
                                 unsigned long long* __restrict__ keys, SelState* st, unsigned long long k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        st->prefix = 0; st->mask = 0; st->krem = k; st->count = 0;
    }
    if (i < 256) st->hist[i] = 0;
    if (i >= P) return;
    unsigned int o = ord32(s[i]);
    if (largest) o = ~o;
    keys[i] = ((unsigned long long)o << 32) | (unsigned long long)(unsigned int)i;
}

__global__ __launch_bounds__(256) void hist_kernel(const unsigned long long* __restrict__ keys, long long P,
                                                   SelState* st, int shift) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long prefix = st->prefix, mask = st->mask;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
        const unsigned long long kx = keys[i];
        if ((kx & mask) == prefix) atomicAdd(&h[(kx >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

__global__ void scan_kernel(SelState* st, int shift) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long k = st->krem, cum = 0;
    int d = 0;
    for (; d < 256; ++d) {
        const unsigned long long c = st->hist[d];
        if (cum + c >= k) break;
        cum += c;
    }
    if (d > 255) d = 255;
    st->krem = k - cum;
    st->prefix |= (unsigned long long)d << shift;
    st->mask |= 255ull << shift;
    for (int i = 0; i < 256; ++i) st->hist[i] = 0;
}

__global__ void compact_kernel(const unsigned long long* __restrict__ keys, long long P, SelState* st,
                               unsigned long long* __restrict__ out, unsigned int cap) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const unsigned long long kx = keys[i];
    if (kx <= st->prefix) {
        const unsigned int slot = atomicAdd(&st->count, 1u);
        if (slot < cap) out[slot] = kx;
    }
}

__global__ void pad_kernel(unsigned long long* out, unsigned int k, unsigned int n2) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k && i < n2) out[i] = ~0ull;
}

constexpr int CHUNK = 4096;   // keys sorted per workgroup in LDS (32 KB)

__device__ __forceinline__ void cmpx(unsigned long long* s, unsigned int i, unsigned int j, bool asc) {
    const unsigned long long a = s[i], b = s[j];
    if ((a > b) == asc) { s[i] = b; s[j] = a; }
}

// sizes 2 .. min(n2, CHUNK): full bitonic build inside LDS
__global__ __launch_bounds__(256) void bitonic_local_sort(unsigned long long* keys, unsigned int n2) {
    __shared__ unsigned long long s[CHUNK];
    const unsigned int base = blockIdx.x * CHUNK, n = min((unsigned int)CHUNK, n2);
    for (unsigned int i = threadIdx.x; i < n; i += 256) s[i] = keys[base + i];
    __syncthreads();
    for (unsigned int size = 2; size <= n; size <<= 1)
        for (unsigned int stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned int t = threadIdx.x; t < n / 2; t += 256) {
                const unsigned int i = 2 * t - (t & (stride - 1)), j = i + stride;
                cmpx(s, i, j, ((base + i) & size) == 0);
            }
            __syncthreads();
        }
    for (unsigned int i = threadIdx.x; i < n; i += 256) keys[base + i] = s[i];
}
__global__ void bitonic_global_step(unsigned long long* keys, unsigned int n2, unsigned int size,
                                    unsigned int stride) {
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n2 / 2) return;
    const unsigned int i = 2 * t - (t & (stride - 1)), j = i + stride;
    const unsigned long long a = keys[i], b = keys[j];
    const bool asc = (i & size) == 0;
    if ((a > b) == asc) { keys[i] = b; keys[j] = a; }
}
// strides CHUNK/2 .. 1 of the merge for `size`
__global__ __launch_bounds__(256) void bitonic_local_merge(unsigned long long* keys, unsigned int size) {
    __shared__ unsigned long long s[CHUNK];
    const unsigned int base = blockIdx.x * CHUNK;
    for (unsigned int i = threadIdx.x; i < CHUNK; i += 256) s[i] = keys[base + i];
    __syncthreads();
    for (unsigned int stride = CHUNK >> 1; stride > 0; stride >>= 1) {
        for (unsigned int t = threadIdx.x; t < CHUNK / 2; t += 256) {
            const unsigned int i = 2 * t - (t & (stride - 1)), j = i + stride;
            cmpx(s, i, j, ((base + i) & size) == 0);
        }
        __syncthreads();
    }
    for (unsigned int i = threadIdx.x; i < CHUNK; i += 256) keys[base + i] = s[i];
}

__global__ void emit_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ scores,
                            int k, int32_t* __restrict__ idx, float* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const unsigned int id = (unsigned int)(keys[i] & 0xffffffffull);
    idx[i] = (int32_t)id;
    if (vals) vals[i] = scores[id];
}

// ---- identification: one row reduction per probe over a (P, G, C) score array (code/ALINK_MTP.py:285-287) -----------------
// A candidate is (value, index); `a` yields to `b` when b is strictly larger, or equal with the lower index: the first maximum
// of the row whatever order the candidates meet in.  A NaN compares false both ways and never enters.
struct IdCand { float v; int i; };
__device__ __forceinline__ IdCand id_better(IdCand a, IdCand b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ IdCand id_wave_max(IdCand a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        IdCand b;
        b.v = __shfl_xor(a.v, o, 64);
        b.i = __shfl_xor(a.i, o, 64);
        a = id_better(a, b);
    }
    return a;
}
__device__ __forceinline__ int id_wave_sum(int c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
}
constexpr int ID_NONE = 0x7fffffff;   // index of a candidate that has seen nothing larger than -inf

// workgroup = a probe row (grid-strided over the rows), thread = gallery entries tid, tid + 256, ...: ascending inside a thread,
// so `>` keeps a thread's first maximum; waves reduce by lane exchange, the four wave results meet in LDS.
__global__ __launch_bounds__(256) void identify_rows_kernel(const float* __restrict__ scores, int P, int G, int C, int col,
                                                            const int32_t* __restrict__ truth, int32_t* __restrict__ flat_argmax,
                                                            int32_t* __restrict__ best, int32_t* __restrict__ rank) {
    __shared__ IdCand s_flat[4], s_best[4];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int p = blockIdx.x; p < P; p += gridDim.x) {
        const float* row = scores + (size_t)p * G * C;
        const int t = (rank && truth) ? truth[p] : -1;
        const bool ranked = t >= 0 && t < G;                       // (uniform over the workgroup)
        const float tv = ranked ? row[(size_t)t * C + col] : 0.f;   // never read outside the row
        IdCand f{-INFINITY, ID_NONE}, b{-INFINITY, ID_NONE};
        int cnt = 0;
        for (int g = tid; g < G; g += 256) {
            const float* e = row + (size_t)g * C;
            for (int c = 0; c < C; ++c) {
                const float v = e[c];
                if (v > f.v) { f.v = v; f.i = g * C + c; }
            }
            const float v = e[col];
            if (v > b.v) { b.v = v; b.i = g; }
            cnt += (ranked && (v > tv || (v == tv && g < t))) ? 1 : 0;
        }
        f = id_wave_max(f);
        b = id_wave_max(b);
        cnt = id_wave_sum(cnt);
        if (lane == 0) { s_flat[wave] = f; s_best[wave] = b; s_cnt[wave] = cnt; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) { f = id_better(f, s_flat[w]); b = id_better(b, s_best[w]); cnt += s_cnt[w]; }
            // nothing above -inf in the row (all -inf / NaN): index 0, np.argmax's answer for a constant row
            if (flat_argmax) flat_argmax[p] = f.i == ID_NONE ? 0 : f.i;
            if (best) best[p] = b.i == ID_NONE ? 0 : b.i;
            if (rank) rank[p] = ranked ? cnt : -1;
        }
        __syncthreads();                                           // the LDS slots are free for the next row
    }
}

// ---- committee disagreement (modAL.disagreement: vote entropy, consensus entropy, maximum KL; code/learners.py:12,287) ---------
// thread = a pair (grid-strided over the pairs): its C contiguous floats of every member's slab, so neighbouring lanes read
// neighbouring rows; VEC floats per load where C and the slabs' alignment allow.  Everything a pair needs lives in registers:
// the members' running sum s[CMAX] (CMAX = the power of two at or above C, every class loop unrolled over it under the
// wave-uniform guard c < C) and the vote counts, one byte per class (M <= 64 fits) in CMAX / 4 words.  The KL term needs the
// finished sum, so the members' rows are read a second time: the same lines by the same lane, one M-row sweep later.
struct DisagreeArgs {
    const float* probs[ALINK_DISAGREE_MAX_MEMBERS];
    int M, C;
    long long P;
    float *vote_entropy, *consensus_entropy, *max_disagreement, *consensus;
    int32_t* votes;
};

template <int CMAX, int VEC>
__device__ __forceinline__ void disagree_load_row(const float* __restrict__ row, int C, float (&x)[CMAX]) {
#pragma unroll
    for (int c = 0; c < CMAX; c += VEC) {
        if (c < C) {                                 // C is a multiple of VEC: c < C covers c .. c + VEC - 1
            if constexpr (VEC == 4) {
                const float4 v = *(const float4*)(row + c);
                x[c] = v.x; x[c + 1] = v.y; x[c + 2] = v.z; x[c + 3] = v.w;
            } else if constexpr (VEC == 2) {
                const float2 v = *(const float2*)(row + c);
                x[c] = v.x; x[c + 1] = v.y;
            } else {
                x[c] = row[c];
            }
        }
    }
}

template <int CMAX, int VEC>
__global__ __launch_bounds__(256) void disagreement_kernel(const DisagreeArgs a) {
#pragma clang fp contract(off)      // the two bit-equalities (head.hip's committee epilogue, score_kernel's entropy) are sums of rounded products
    constexpr int NW = CMAX >= 4 ? CMAX / 4 : 1;
    const int M = a.M, C = a.C;
    const float Mf = (float)M;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.P; i += stride) {
        float s[CMAX], x[CMAX];
        unsigned int cnt[NW];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) s[c] = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) cnt[w] = 0u;
        for (int m = 0; m < M; ++m) {
            disagree_load_row<CMAX, VEC>(a.probs[m] + i * C, C, x);
            float best = -INFINITY;                 // `>`: the first maximum, and a NaN never wins (alink_identify_rows)
            int vote = 0;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if (c < C) {
                    if (x[c] > best) { best = x[c]; vote = c; }
                    s[c] = m == 0 ? x[c] : s[c] + x[c];     // (p_0 + p_1) + ... in member order
                }
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) cnt[w] += (vote >> 2) == w ? 1u << ((vote & 3) * 8) : 0u;
            if (a.votes) a.votes[i * M + m] = vote;
        }
        if (a.vote_entropy) {
            // a function of the MULTISET of counts: sum over v = 1 .. M, ascending, of (classes holding v votes) x t_v
            float e = 0.f;
            for (int v = 1; v <= M; ++v) {
                int k = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w)
#pragma unroll
                    for (int b = 0; b < 4; ++b) k += ((cnt[w] >> (8 * b)) & 255u) == (unsigned)v ? 1 : 0;
                if (k) {
                    const float f = (float)v / Mf;
                    const float t = -f * logf(f);
                    e += (float)k * t;
                }
            }
            a.vote_entropy[i] = e;
        }
        if (a.consensus || a.consensus_entropy) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) x[c] = s[c] / Mf;        // one IEEE division: head.hip's final_div
            if (a.consensus) {
                float* o = a.consensus + i * C;
#pragma unroll
                for (int c = 0; c < CMAX; c += VEC) {
                    if (c < C) {
                        if constexpr (VEC == 4) *(float4*)(o + c) = make_float4(x[c], x[c + 1], x[c + 2], x[c + 3]);
                        else if constexpr (VEC == 2) *(float2*)(o + c) = make_float2(x[c], x[c + 1]);
                        else o[c] = x[c];
                    }
                }
            }
            if (a.consensus_entropy) {              // score_kernel's entropy branch, operation for operation
                float t = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) t += x[c];
                float e = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c < C) {
                        const float q = x[c] / t;
                        e += (q > 0.f) ? -q * logf(q) : 0.f;
                    }
                }
                a.consensus_entropy[i] = e;
            }
        }
        if (a.max_disagreement) {
            float worst = 0.f;
            for (int m = 0; m < M; ++m) {
                disagree_load_row<CMAX, VEC>(a.probs[m] + i * C, C, x);
                float r = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) r += x[c];
                float kl = 0.f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c < C) {
                        const float ph = x[c] / r;
                        // against the members' SUM: s >= every addend, so the ratio stays at or below M (1 + rounding)
                        kl += (ph > 0.f) ? ph * logf(ph * Mf / s[c]) : 0.f;
                    }
                }
                worst = m == 0 ? kl : fmaxf(worst, kl);
            }
            a.max_disagreement[i] = worst;
        }
    }
}

template <int CMAX>
void launch_disagreement(int vec, unsigned blocks, hipStream_t st, const DisagreeArgs& a) {
    if constexpr (CMAX >= 4) {
        if (vec == 4) { hipLaunchKernelGGL((disagreement_kernel<CMAX, 4>), dim3(blocks), dim3(256), 0, st, a); return; }
    }
    if (vec >= 2) hipLaunchKernelGGL((disagreement_kernel<CMAX, 2>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((disagreement_kernel<CMAX, 1>), dim3(blocks), dim3(256), 0, st, a);
}

unsigned int next_pow2(unsigned int x) {
    unsigned int p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace
}  // namespace alink

using namespace alink;

extern "C" {

int alink_score(int kind, const float* dev_probs, const float* dev_b, int col, int64_t P, int C,
                float* dev_scores, void* stream) {
    ALINK_REQUIRE(dev_probs && dev_scores, ALINK_EINVAL, "NULL argument");
    DeviceGuard dg(device_of_pointer(dev_probs));
    ALINK_REQUIRE(kind >= 0 && kind <= 3, ALINK_EINVAL, "unknown score kind %d", kind);
    ALINK_REQUIRE(C >= 1, ALINK_EINVAL, "C must be >= 1");
    ALINK_REQUIRE(kind != ALINK_SCORE_DISPARITY || (dev_b && col >= 0 && col < C), ALINK_EINVAL,
                  "disparity needs dev_b and 0 <= col < C");
    if (P == 0) return ALINK_OK;
    ALINK_REQUIRE(P > 0, ALINK_EINVAL, "negative P");
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kind,
                       dev_probs, dev_b, col, (long long)P, C, dev_scores);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

int alink_committee_disagreement(const float* const* dev_member_probs, int n_members, int64_t P, int C, float* dev_vote_entropy,
                                 float* dev_consensus_entropy, float* dev_max_disagreement, float* dev_consensus,
                                 int32_t* dev_votes, void* stream) {
    ALINK_REQUIRE(n_members >= 1 && n_members <= ALINK_DISAGREE_MAX_MEMBERS, ALINK_EINVAL, "n_members=%d outside 1..%d", n_members,
                  ALINK_DISAGREE_MAX_MEMBERS);
    ALINK_REQUIRE(C >= 2 && C <= ALINK_DISAGREE_MAX_CLASSES, ALINK_EINVAL, "C=%d outside 2..%d", C, ALINK_DISAGREE_MAX_CLASSES);
    ALINK_REQUIRE(P >= 0, ALINK_EINVAL, "negative P");
    if (P == 0 || (!dev_vote_entropy && !dev_consensus_entropy && !dev_max_disagreement && !dev_consensus && !dev_votes)) return ALINK_OK;
    ALINK_REQUIRE(dev_member_probs, ALINK_EINVAL, "NULL member array");
    DisagreeArgs a;
    uintptr_t bits = (uintptr_t)dev_consensus;       // every address a vector access starts from
    for (int m = 0; m < ALINK_DISAGREE_MAX_MEMBERS; ++m) {
        a.probs[m] = m < n_members ? dev_member_probs[m] : nullptr;
        ALINK_REQUIRE(m >= n_members || a.probs[m], ALINK_EINVAL, "NULL probabilities of member %d", m);
        bits |= (uintptr_t)a.probs[m];
    }
    DeviceGuard dg(device_of_pointer(a.probs[0]));
    a.M = n_members; a.C = C; a.P = (long long)P;
    a.vote_entropy = dev_vote_entropy; a.consensus_entropy = dev_consensus_entropy; a.max_disagreement = dev_max_disagreement;
    a.consensus = dev_consensus; a.votes = dev_votes;
    const int vec = (C % 4 == 0 && bits % 16 == 0) ? 4 : (C % 2 == 0 && bits % 8 == 0) ? 2 : 1;
    const long long nb = (P + 255) / 256;
    const unsigned blocks = nb < 65536 ? (unsigned)nb : 65536u;     // the kernel strides over the pairs
    hipStream_t st = (hipStream_t)stream;
    if (C <= 2) launch_disagreement<2>(vec, blocks, st, a);
    else if (C <= 4) launch_disagreement<4>(vec, blocks, st, a);
    else if (C <= 8) launch_disagreement<8>(vec, blocks, st, a);
    else if (C <= 16) launch_disagreement<16>(vec, blocks, st, a);
    else launch_disagreement<32>(vec, blocks, st, a);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

int alink_identify_rows(const float* dev_scores, int P, int G, int C, int col, const int32_t* dev_true,
                        int32_t* dev_flat_argmax, int32_t* dev_best, int32_t* dev_rank, void* stream) {
    ALINK_REQUIRE(P >= 0 && G >= 1 && C >= 1 && col >= 0 && col < C, ALINK_EINVAL, "bad shape (P=%d, G=%d, C=%d, col=%d)", P, G, C, col);
    ALINK_REQUIRE((long long)G * C < (1ll << 31), ALINK_EINVAL, "G * C = %lld does not fit the int32 flattened index", (long long)G * C);
    ALINK_REQUIRE(!dev_rank || dev_true, ALINK_EINVAL, "dev_rank needs dev_true");
    if (P == 0 || (!dev_flat_argmax && !dev_best && !dev_rank)) return ALINK_OK;
    ALINK_REQUIRE(dev_scores, ALINK_EINVAL, "NULL scores");
    DeviceGuard dg(device_of_pointer(dev_scores));
    const unsigned blocks = P < 65536 ? (unsigned)P : 65536u;     // the kernel strides over the rows
    hipLaunchKernelGGL(identify_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dev_scores, P, G, C, col, dev_true,
                       dev_flat_argmax, dev_best, dev_rank);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

size_t alink_topk_scratch_bytes(int64_t P, int k) {
    if (P <= 0 || k <= 0) return 0;
    const size_t n2 = next_pow2((unsigned int)k);
    return (((size_t)P * 8 + 255) & ~(size_t)255) + ((n2 * 8 + 255) & ~(size_t)255) + 2048;
}

int alink_topk(const float* dev_scores, int64_t P, int k, int largest, int32_t* dev_idx, float* dev_vals,
               void* dev_scratch, void* stream) {
    ALINK_REQUIRE(dev_scores && dev_idx && dev_scratch, ALINK_EINVAL, "NULL argument");
    DeviceGuard dg(device_of_pointer(dev_scores));
    ALINK_REQUIRE(P > 0 && P < (1ll << 31), ALINK_EINVAL, "P=%lld outside 1..2^31-1", (long long)P);
    ALINK_REQUIRE(k > 0 && k <= P, ALINK_EINVAL, "k=%d outside 1..P", k);
    ALINK_REQUIRE(((uintptr_t)dev_scratch & 255) == 0, ALINK_EINVAL, "scratch must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned int n2 = next_pow2((unsigned int)k);
    char* base = (char*)dev_scratch;
    unsigned long long* keys = (unsigned long long*)base;
    unsigned long long* out = (unsigned long long*)(base + (((size_t)P * 8 + 255) & ~(size_t)255));
    SelState* state = (SelState*)((char*)out + (((size_t)n2 * 8 + 255) & ~(size_t)255));
    const unsigned nb = (unsigned)((P + 255) / 256);
    hipLaunchKernelGGL(make_keys_kernel, dim3(nb), dim3(256), 0, st, dev_scores, (long long)P, largest, keys,
                       state, (unsigned long long)k);
    const unsigned hb = nb < 2048 ? nb : 2048;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(hist_kernel, dim3(hb), dim3(256), 0, st, keys, (long long)P, state, shift);
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(64), 0, st, state, shift);
    }
    hipLaunchKernelGGL(compact_kernel, dim3(nb), dim3(256), 0, st, keys, (long long)P, state, out, (unsigned)k);
    if (n2 > (unsigned)k)
        hipLaunchKernelGGL(pad_kernel, dim3((n2 + 255) / 256), dim3(256), 0, st, out, (unsigned)k, n2);
    const unsigned chunks = n2 > CHUNK ? n2 / CHUNK : 1;
    hipLaunchKernelGGL(bitonic_local_sort, dim3(chunks), dim3(256), 0, st, out, n2);
    for (unsigned int size = 2 * CHUNK; size <= n2 && size != 0; size <<= 1) {
        for (unsigned int stride = size >> 1; stride >= CHUNK; stride >>= 1)
            hipLaunchKernelGGL(bitonic_global_step, dim3((n2 / 2 + 255) / 256), dim3(256), 0, st, out, n2, size,
                               stride);
        hipLaunchKernelGGL(bitonic_local_merge, dim3(n2 / CHUNK), dim3(256), 0, st, out, size);
    }
    hipLaunchKernelGGL(emit_kernel, dim3((k + 255) / 256), dim3(256), 0, st, out, dev_scores, k, dev_idx,
                       dev_vals);
    ALINK_HIP(hipGetLastError());
    return ALINK_OK;
}

}  // extern "C"
