// net_host.h — the host-side plumbing the image networks (backbone.hip, resnet50.hip, vgg16.hip) share around their kernels:
// the table of checkpoint tensors, the host number formats, the one walk that packs a convolution's folded weights, and — for
// translation units compiled as HIP — owned device memory, ConvParams geometry, the K-split launch, per-launch timing and the
// split-precision scale calibration.  The first part is plain C++ (no HIP, no device code) and builds with the host compiler
// alone, like conv_kernel.h; the second part needs alink_common.h and is seen by hipcc only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/alink_hip.h"
#include "conv_kernel.h"

namespace alink {

void     set_error(const char* fmt, ...);
uint16_t f32_to_bf16_rne(float f);
uint16_t f32_to_f16_rne(float f);

// ---- host number formats ------------------------------------------------------------------------------------------------
inline uint16_t cvt(int dtype, float f) { return dtype == ALINK_DT_BF16 ? f32_to_bf16_rne(f) : f32_to_f16_rne(f); }
// A folded weight v (real arithmetic, a double) in 16-bit storage.  Direct: the f16 nearest v.  ViaFloat32: v rounded to float32
// first and that to f16 — two roundings, a different last bit for about one value in 2^13.  (bf16 is cut from the float32 either
// way.)  Which of the two a buffer holds is part of what the network computes, so it is said here and not left to what the
// compiler makes of (_Float16)(float)v: the IR backbone's own weights are Direct; the columns of its fused shortcuts and every
// weight of ResNet-50 and VGG-16 are ViaFloat32.
enum class Round16 { Direct, ViaFloat32 };
inline uint16_t cvt(int dtype, double v, Round16 round) {
    if (dtype == ALINK_DT_BF16 || round == Round16::ViaFloat32) return cvt(dtype, (float)v);
    const _Float16 h = (_Float16)v;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
// ALINK_DT_F16X2: x -> f16 pair, hi = RN16(x), lo = RN16(x - hi): |x - hi - lo| <= 2^-22 |x| (while lo stays normal)
inline void split16(double x, uint16_t* hi, uint16_t* lo) {
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (double)h);
    memcpy(hi, &h, 2);
    memcpy(lo, &l, 2);
}
// exponent e with maxabs * 2^e in [1024, 2048): 32x below the f16 overflow threshold, lo = 2^-11 hi still >= 2^-1
inline int scale_exp(double maxabs) {
    if (!(maxabs > 0.0) || !std::isfinite(maxabs)) return 0;
    return 10 - std::ilogb(maxabs);
}

// ---- checkpoint tensors -----------------------------------------------------------------------------------------------------
// The tensors a network expects (name, element count, in load order) and the ones loaded so far.  finalize() reads `raw`
// through at() and clears it.
struct TensorTable {
    std::vector<std::pair<std::string, size_t>> expected;
    std::map<std::string, std::vector<float>> raw;

    void expect(const std::string& name, size_t count) { expected.emplace_back(name, count); }
    int  count() const { return (int)expected.size(); }
    int  info(int i, const char** name, size_t* n) const {
        if (i < 0 || i >= count()) { set_error("tensor index out of range"); return ALINK_EINVAL; }
        if (name) *name = expected[i].first.c_str();
        if (n) *n = expected[i].second;
        return ALINK_OK;
    }
    // what: the network as the "not part of" message calls it; handle: the word of the "already finalized" message
    int load(const char* name, const float* host, size_t n, bool finalized, const char* what, const char* handle = "network") {
        if (!name || !host) { set_error("NULL argument"); return ALINK_EINVAL; }
        if (finalized) { set_error("%s already finalized", handle); return ALINK_ESTATE; }
        for (const auto& e : expected)
            if (e.first == name) {
                if (e.second != n) { set_error("tensor %s: expected %zu elements, got %zu", name, e.second, n); return ALINK_EINVAL; }
                raw[name].assign(host, host + n);
                return ALINK_OK;
            }
        set_error("tensor %s is not part of %s", name, what);
        return ALINK_ENOTFOUND;
    }
    int require_all_loaded() const {
        for (const auto& e : expected)
            if (!raw.count(e.first)) { set_error("tensor %s was never loaded", e.first.c_str()); return ALINK_ESTATE; }
        return ALINK_OK;
    }
    const std::vector<float>& at(const std::string& name) const { return raw.at(name); }
    void clear() { raw.clear(); }
};

// ---- packing a convolution's weights ------------------------------------------------------------------------------------
// The one walk over (output row, tap, input channel) that asks WeightLayout where a value goes.  value(co, tap, ci) is the
// folded weight in real arithmetic (double); shortcut(co, ci2) the fused 1x1 projection's (layouts with cin2 columns).
// 16-bit layouts store cvt(dtype, value, round), and the shortcut's columns ViaFloat32.  Split layouts store the f16 pair of
// value x 2^e_w, e_w from the largest |value| (scale_exp) unless the caller fixes it.
struct PackedWeights {
    std::vector<uint16_t> w;
    int e_w = 0;
};

template <class Value, class Shortcut>
PackedWeights pack_conv_weights(const WeightLayout& wl, int dtype, Round16 round, int rows, Value&& value, Shortcut&& shortcut,
                                const int* fixed_e_w = nullptr) {
    PackedWeights r;
    r.w.resize(wl.size(rows));
    if (wl.split && fixed_e_w) r.e_w = *fixed_e_w;
    if (wl.split && !fixed_e_w) {
        double mx = 0.0;
        for (int co = 0; co < rows; ++co)
            for (int tap = 0; tap < wl.taps; ++tap)
                for (int ci = 0; ci < wl.cin; ++ci) mx = std::max(mx, std::fabs((double)value(co, tap, ci)));
        r.e_w = scale_exp(mx);
    }
    for (int co = 0; co < rows; ++co) {
        for (int tap = 0; tap < wl.taps; ++tap)
            for (int ci = 0; ci < wl.cin; ++ci) {
                const double v = value(co, tap, ci);
                const size_t at = wl.at(co, tap, ci);
                if (wl.split) split16(std::ldexp(v, r.e_w), &r.w[at], &r.w[at + wl.lo_offset()]);
                else          r.w[at] = cvt(dtype, v, round);
            }
        for (int ci = 0; ci < wl.cin2; ++ci) r.w[wl.at_shortcut(co, ci)] = cvt(dtype, (double)shortcut(co, ci), Round16::ViaFloat32);
    }
    return r;
}
template <class Value>
PackedWeights pack_conv_weights(const WeightLayout& wl, int dtype, Round16 round, int rows, Value&& value) {
    return pack_conv_weights(wl, dtype, round, rows, value, [](int, int) { return 0.0; });
}

// The weights of the backward (input-gradient) convolution, transposed and flipped: Wb[ci][tap'][co] = value(co, k*k-1-tap', ci).
// bl is the layout with the roles exchanged (rows = the forward Cin, bl.cin = the forward Cout); value as for the forward.
template <class Value>
std::vector<uint16_t> pack_conv_weights_backward(const WeightLayout& bl, int dtype, Round16 round, int rows, Value&& value) {
    return pack_conv_weights(bl, dtype, round, rows, [&](int ci, int tap, int co) { return value(co, bl.taps - 1 - tap, ci); }).w;
}

}  // namespace alink

#ifdef __HIPCC__
#include "alink_common.h"

namespace alink {

// ---- owned device memory ------------------------------------------------------------------------------------------------
// Device pointers a handle owns; freed with it.
class DeviceAllocs {
    std::vector<void*> ptrs;

  public:
    DeviceAllocs() = default;
    DeviceAllocs(const DeviceAllocs&) = delete;
    DeviceAllocs& operator=(const DeviceAllocs&) = delete;
    ~DeviceAllocs() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    void adopt(void* p) { ptrs.push_back(p); }
    int  alloc(size_t bytes, void** d) {
        ALINK_HIP(hipMalloc(d, bytes));
        ptrs.push_back(*d);
        return ALINK_OK;
    }
    int zeros(size_t bytes, void** d) {
        const int rc = alloc(bytes, d);
        if (rc) return rc;
        ALINK_HIP(hipMemset(*d, 0, bytes));
        return ALINK_OK;
    }
    template <typename V>
    int upload(const std::vector<V>& h, void** d) {
        const int rc = alloc(h.size() * sizeof(V), d);
        if (rc) return rc;
        ALINK_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(V), hipMemcpyHostToDevice));
        return ALINK_OK;
    }
};

// ---- launch geometry ----------------------------------------------------------------------------------------------------
// The geometry of one convolution launch, and the one statement of how many K-steps it walks: a step per tap and 64 input
// channels (three products per step in split precision), then the steps of a fused shortcut's Cin2 channels.  A backward
// convolution is the same call with Cin and Cout exchanged, on the output grid, at stride 1.
inline void conv_geometry(ConvParams& p, int N, int H, int W, int Cin, int Cout, int ksz, int stride, int pad, int Cin2 = 0,
                          bool x2 = false) {
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.ksz = ksz; p.stride = stride; p.pad = pad;
    p.Ho = (H + 2 * pad - ksz) / stride + 1;
    p.Wo = (W + 2 * pad - ksz) / stride + 1;
    p.M = N * p.Ho * p.Wo;
    p.splitk = 1;
    p.ksteps_per_split = ksz * ksz * (Cin / 64) * (x2 ? 3 : 1) + Cin2 / 64;
}
// a prebuilt ConvParams (geometry at N = 0) for a batch of N images
inline void with_batch(ConvParams& p, int N) { p.N = N; p.M = N * p.Ho * p.Wo; }

// ---- K-split launch -------------------------------------------------------------------------------------------------------
// what is launched for p: p itself, or (S > 1) its K walk divided over S workgroup rows that leave f32 slabs of raw sums
inline ConvParams k_split_of(const ConvParams& p, int S, void* slabs) {
    ConvParams q = p;
    if (S > 1) { q.out = slabs; q.splitk = S; q.ksteps_per_split = p.ksteps_per_split / S; }
    return q;
}
// the launch itself: fused, or the S slabs and the finish kernel that sums them in order and applies p's epilogue
inline hipError_t launch_conv_maybe_split(ConvKernel kernel, int dtype, const ConvParams& p, int S, void* slabs, hipStream_t st) {
    hipError_t e = launch_conv(kernel, dtype, k_split_of(p, S, slabs), st);
    if (e == hipSuccess && S > 1) e = launch_conv_split_finish(dtype, p, (const float*)slabs, S, st);
    return e;
}

// Which kernel serves launch_conv(k, dtype, q): the launchers' own hand-off predicates on the ConvParams that is launched.
// 0 = kernel k itself, 1 = conv3x3_lat_kernel, 2 = conv_gemm_lat_kernel.
inline int served_form(ConvKernel k, int dtype, const ConvParams& q) {
    if (k == ConvKernel::Igemm) return conv_gemm_lat_applies(dtype, q) ? 2 : 0;          // launch_conv_igemm
    if (traits(k).channel_block) return conv3x3_lat_applies(dtype, q) ? 1 : 0;           // launch_conv3x3_linear
    return 0;
}

// ---- per-launch timing ----------------------------------------------------------------------------------------------------
// Events around the launches of a profiled call; destroyed with the object on every return path.
class LaunchTimer {
    bool on;
    std::vector<hipEvent_t> ev;

  public:
    explicit LaunchTimer(bool on_) : on(on_) {}
    LaunchTimer(const LaunchTimer&) = delete;
    LaunchTimer& operator=(const LaunchTimer&) = delete;
    ~LaunchTimer() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int mark(hipStream_t stream) {
        if (!on) return ALINK_OK;
        hipEvent_t e;
        ALINK_HIP(hipEventCreate(&e));
        ev.push_back(e);
        ALINK_HIP(hipEventRecord(e, stream));
        return ALINK_OK;
    }
    int intervals() const { return ev.empty() ? 0 : (int)ev.size() - 1; }
    // ms[i] = milliseconds between mark i and mark i + 1, over reps, for the first `cap` intervals (the stream is synchronised)
    int elapsed(float* ms, int cap, int reps = 1) const {
        for (int i = 0; i < intervals() && i < cap; ++i) {
            float t = 0.f;
            ALINK_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            ms[i] = t / (float)reps;
        }
        return ALINK_OK;
    }
};

// ---- split-precision calibration and the range flag ---------------------------------------------------------------------
// ALINK_DT_F16X2 stores every tensor as f16 pairs x 2^e.  The exponents of the outputs are chosen by a calibration run
// (settle); a forward in 16-bit storage that leaves the range raises the pinned flag word its last kernel is handed.
struct ScaleCalibration {
    unsigned* d_absmax = nullptr;   // calibration scratch: bits of the largest |value| of a tensor (split precision only)
    bool calibrated = false;
    int* h_flag = nullptr;          // pinned, device-visible: raised when a result is not finite
    int* d_flag = nullptr;          // the same word as the device addresses it

    ScaleCalibration() = default;
    ScaleCalibration(const ScaleCalibration&) = delete;
    ScaleCalibration& operator=(const ScaleCalibration&) = delete;
    ~ScaleCalibration() {
        if (h_flag) (void)hipHostFree(h_flag);
    }
    int init(DeviceAllocs& mem, bool x2) {
        if (x2) {
            const int rc = mem.alloc(256, (void**)&d_absmax);
            if (rc) return rc;
        }
        ALINK_HIP(hipHostMalloc((void**)&h_flag, 64, hipHostMallocMapped));
        *h_flag = 0;
        ALINK_HIP(hipHostGetDevicePointer((void**)&d_flag, h_flag, 0));
        return ALINK_OK;
    }
    // Runs launch(e) with the output exponent e = *e_io.  calib 0: once, a normal forward.  calib 1: again until the largest
    // |output| lies in [1024, 2048) (f16 pairs: 32x below overflow, lo halves normal) — a power-of-two scale changes no bit of
    // the result, only where it sits; calib 2: the same, never above the exponent already held.  Synchronous when calib != 0.
    template <class Launch>
    int settle(int calib, int* e_io, const void* out, size_t n_elems, hipStream_t stream, Launch&& launch) {
        int e = *e_io;
        for (int attempt = 0; attempt < 24; ++attempt) {
            const int rcl = launch(e);
            if (rcl) return rcl;
            if (!calib) break;
            unsigned bits = 0;
            ALINK_HIP(hipMemsetAsync(d_absmax, 0, 4, stream));
            ALINK_HIP(launch_absmax_f16(out, n_elems, d_absmax, stream));
            ALINK_HIP(hipMemcpyAsync(&bits, d_absmax, 4, hipMemcpyDeviceToHost, stream));
            ALINK_HIP(hipStreamSynchronize(stream));
            float m;
            memcpy(&m, &bits, 4);
            if (bits >= 0x7f800000u) { e -= 8; continue; }                 // left the range: lower the scale and redo
            if (m == 0.f) break;
            int want = e + (10 - std::ilogb(m));
            if (calib == 2 && calibrated) want = std::min(want, *e_io);
            if (want == e) break;
            e = want;
        }
        *e_io = e;
        return ALINK_OK;
    }
    int range_flag(int reset) {
        if (!h_flag) return 0;
        const int v = *(volatile int*)h_flag != 0 ? 1 : 0;
        if (reset) *(volatile int*)h_flag = 0;
        return v;
    }
    // Clears the flag for a calibration run; a report still pending from an earlier forward (lazy range checks read the flag
    // later) is put back when the guard goes.
    struct PendingReport {
        int* f;
        int  v;
        explicit PendingReport(ScaleCalibration& c) : f(c.h_flag), v(*(volatile int*)c.h_flag) { *f = 0; }
        PendingReport(const PendingReport&) = delete;
        ~PendingReport() {
            if (v) *(volatile int*)f = 1;
        }
    };
    // alink_<net>_get_scales / _set_scales behind the entry's own "before finalize" check: at(i) is exponent i of the network,
    // `item` what the network calls the thing an exponent belongs to
    template <class At>
    int get_scales(const char* net, bool x2, int count, At&& at, int* exponents, int n) const {
        ALINK_REQUIRE(x2, ALINK_ESTATE, "only the split-precision mode (ALINK_DT_F16X2) has scales");
        ALINK_REQUIRE(calibrated, ALINK_ESTATE, "alink_%s_get_scales before alink_%s_calibrate / set_scales", net, net);
        ALINK_REQUIRE(exponents && n == count, ALINK_EINVAL, "expected room for %d exponents, got %d", count, n);
        for (int i = 0; i < count; ++i) exponents[i] = at(i);
        return ALINK_OK;
    }
    template <class At>
    int set_scales(const char* item, bool x2, int count, At&& at, const int* exponents, int n) {
        ALINK_REQUIRE(x2, ALINK_ESTATE, "only the split-precision mode (ALINK_DT_F16X2) has scales");
        ALINK_REQUIRE(exponents && n == count, ALINK_EINVAL, "expected %d exponents, got %d", count, n);
        for (int i = 0; i < n; ++i)
            ALINK_REQUIRE(exponents[i] >= -126 && exponents[i] <= 126, ALINK_EINVAL, "exponent %d of %s %d is not a float32 power of two",
                          exponents[i], item, i);
        for (int i = 0; i < count; ++i) at(i) = exponents[i];
        calibrated = true;
        return ALINK_OK;
    }
};

}  // namespace alink
#endif  // __HIPCC__
