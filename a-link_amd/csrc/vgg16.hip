// vgg16.hip — the VGGFace VGG-16 feature extractor behind siamese.FaceVGG16
// (reference code/siamese.py:187-200: keras_vggface VGGFace(model='vgg16', include_top=False), output
// of 'pool5' flattened -> 25088-d; preprocess = utils.preprocess_input(version=1)).
//
// keras-vggface 0.5 (reference requirements.txt:19) is not vendored; the graph restated here is its
// VGG16 (keras_vggface/models.py): thirteen 3x3 'same' convolutions WITH bias + ReLU in five blocks of
// widths 64, 128, 256, 512, 512 (2, 2, 3, 3, 3 layers), each block closed by MaxPooling2D((2,2), 2);
// Flatten of the 7 x 7 x 512 pool5 map is (h, w, c)-major.  preprocess_input(version=1): RGB -> BGR,
// subtract (93.5940, 104.7624, 129.1863) per BGR channel.
//
// conv1_1 (3 -> 64) is the IR backbone's K = 27 MFMA stem kernel with this network's normalisation in
// its loader; every other convolution runs on conv3x3_direct / conv_igemm (bias as the folded-BN
// bias slot, ReLU as a zero-slope PReLU epilogue).  New here: the 2x2 max-pool, whose last instance
// writes the float32 features.
#include "conv_device.h"
#include "net_host.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace alink {
namespace {

// MaxPooling2D((2,2), strides 2) on NHWC T (floor on odd sizes); OUT = T, or float for the last pool
template <typename T, typename OUT>
__global__ void maxpool2_kernel(const T* __restrict__ in, OUT* __restrict__ out, int N, int H, int W, int C) {
    typedef typename Vec8<T>::type vec8;
    const int Ho = H / 2, Wo = W / 2, c8n = C >> 3;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * Ho * Wo * c8n) return;
    const int c8 = (int)(i % c8n);
    long long t = i / c8n;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int n = (int)(t / Ho);
    const T* base = in + (((size_t)n * H + 2 * oy) * W + 2 * ox) * C + c8 * 8;
    const vec8 a = *(const vec8*)base, b = *(const vec8*)(base + C);
    const vec8 c = *(const vec8*)(base + (size_t)W * C), d = *(const vec8*)(base + (size_t)W * C + C);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float m = max_keep_nan(max_keep_nan((float)a[j], (float)b[j]), max_keep_nan((float)c[j], (float)d[j]));
        out[(size_t)i * 8 + j] = (OUT)m;
    }
}

const int kBlocks[5] = {2, 2, 3, 3, 3};
const int kWidth[5] = {64, 128, 256, 512, 512};

struct VOp {
    int kind;          // 0 stem (conv1_1), 1 conv, 2 pool
    ConvParams cp;
    ConvKernel kernel = ConvKernel::Igemm;
    int in_buf = 0, out_buf = 0, H = 0, W = 0, C = 0;
    std::string name;
};

}  // namespace
}  // namespace alink

using namespace alink;

struct alink_vgg16 {
    int device = -1;
    int H, W, dtype;
    TensorTable tensors;
    bool finalized = false;
    DeviceAllocs mem;
    std::vector<VOp> ops;
    void* d_stem_w = nullptr;
    float *d_stem_bias = nullptr, *d_zero_alpha = nullptr;
    void* d_zero = nullptr;
    int Hf = 0, Wf = 0;
    size_t buf_elems_per_image = 0;
};

namespace {

std::string lname(int b, int l) {
    char s[32];
    snprintf(s, sizeof(s), "conv%d_%d", b + 1, l + 1);
    return s;
}

}  // namespace

extern "C" {

alink_vgg16_t* alink_vgg16_create(int height, int width, int dtype) {
    if (dtype != ALINK_DT_BF16 && dtype != ALINK_DT_F16) { set_error("bad dtype"); return nullptr; }
    if (height < 32 || width < 32 || height > 512 || width > 512) { set_error("input %dx%d unsupported", height, width); return nullptr; }
    alink_vgg16* r = new alink_vgg16();
    r->device = current_device();
    r->H = height; r->W = width; r->dtype = dtype;
    int cin = 3;
    for (int b = 0; b < 5; ++b)
        for (int l = 0; l < kBlocks[b]; ++l) {
            r->tensors.expect(lname(b, l) + "/kernel", (size_t)9 * cin * kWidth[b]);
            r->tensors.expect(lname(b, l) + "/bias", (size_t)kWidth[b]);
            cin = kWidth[b];
        }
    r->Hf = height >> 5; r->Wf = width >> 5;
    return r;
}

void alink_vgg16_destroy(alink_vgg16_t* r) {
    if (!r) return;
    DeviceGuard dg(r->device);
    delete r;
}
int alink_vgg16_num_tensors(const alink_vgg16_t* r) { return r ? r->tensors.count() : 0; }
int alink_vgg16_tensor_info(const alink_vgg16_t* r, int i, const char** name, size_t* count) {
    ALINK_REQUIRE(r, ALINK_EINVAL, "tensor index out of range");
    return r->tensors.info(i, name, count);
}
int alink_vgg16_feature_size(const alink_vgg16_t* r) { return r ? r->Hf * r->Wf * 512 : 0; }

int alink_vgg16_load(alink_vgg16_t* r, const char* name, const float* host, size_t count) {
    ALINK_REQUIRE(r, ALINK_EINVAL, "NULL argument");
    return r->tensors.load(name, host, count, r->finalized, "the VGGFace VGG-16");
}

int alink_vgg16_finalize(alink_vgg16_t* r) {
    ALINK_REQUIRE(r && !r->finalized, ALINK_ESTATE, "bad state");
    DeviceGuard dg(r->device);
    int rc = r->tensors.require_all_loaded();
    if (rc) return rc;
    if ((rc = init_kernels())) return rc;
    if ((rc = r->mem.zeros(4096, &r->d_zero))) return rc;
    if ((rc = r->mem.zeros(512 * 4, (void**)&r->d_zero_alpha))) return rc;
    {   // conv1_1: [64'][64] T, k = ky*16 + kx*3 + c (StemParams::wgt) from the Keras kernel (3,3,3,64)
        const auto& w = r->tensors.at("conv1_1/kernel");
        std::vector<uint16_t> wq((size_t)64 * 64, cvt(r->dtype, 0.f));
        for (int co = 0; co < 64; ++co)
            for (int k = 0; k < 27; ++k)
                wq[(size_t)perm64_row_of_channel(co) * 64 + (k / 9) * 16 + k % 9] = cvt(r->dtype, w[(size_t)k * 64 + co]);
        if ((rc = r->mem.upload(wq, &r->d_stem_w))) return rc;
        if ((rc = r->mem.upload(r->tensors.at("conv1_1/bias"), (void**)&r->d_stem_bias))) return rc;
    }
    int H = r->H, W = r->W, cin = 64, cur = 0;
    r->buf_elems_per_image = (size_t)H * W * 64;
    VOp st; st.kind = 0; st.out_buf = 0; st.H = H; st.W = W; st.name = "conv1_1"; r->ops.push_back(st);
    for (int b = 0; b < 5; ++b) {
        for (int l = (b == 0 ? 1 : 0); l < kBlocks[b]; ++l) {
            const int cout = kWidth[b];
            const auto& w = r->tensors.at(lname(b, l) + "/kernel");       // (3, 3, cin, cout)
            VOp op; op.kind = 1; op.name = lname(b, l);
            op.kernel = direct_variant_tiles(3, 1, 1, H, W, cin, cout);
            const std::vector<uint16_t> wq =
                pack_conv_weights(weight_layout(op.kernel, 3, cin), r->dtype, Round16::ViaFloat32, cout,
                                  [&](int co, int tap, int ci) { return (double)w[((size_t)tap * cin + ci) * cout + co]; }).w;
            void* d_w = nullptr;
            float* d_b = nullptr;
            if ((rc = r->mem.upload(wq, &d_w))) return rc;
            if ((rc = r->mem.upload(r->tensors.at(lname(b, l) + "/bias"), (void**)&d_b))) return rc;
            ConvParams& p = op.cp;
            memset(&p, 0, sizeof(p));
            p.wgt = d_w; p.bias = d_b; p.alpha = r->d_zero_alpha; p.zero = r->d_zero;
            conv_geometry(p, 0, H, W, cin, cout, 3, 1, 1);       // N, M: with_batch, per call
            op.in_buf = cur; op.out_buf = cur ^ 1; cur ^= 1;
            r->ops.push_back(op);
            r->buf_elems_per_image = std::max(r->buf_elems_per_image, (size_t)H * W * cout);
            cin = cout;
        }
        VOp mp; mp.kind = 2; mp.in_buf = cur; mp.out_buf = cur ^ 1; mp.H = H; mp.W = W; mp.C = cin; mp.name = "pool" + std::to_string(b + 1);
        cur ^= 1;
        r->ops.push_back(mp);
        H /= 2; W /= 2;
    }
    r->tensors.clear();
    r->finalized = true;
    return ALINK_OK;
}

size_t alink_vgg16_workspace_bytes(const alink_vgg16_t* r, int n_images) {
    if (!r || !r->finalized || n_images <= 0) return 0;
    const size_t one = ((size_t)n_images * r->buf_elems_per_image * 2 + 255) & ~(size_t)255;
    return 2 * one;
}

// ops [0, n_ops) of the network on the caller's workspace: alink_vgg16_embed's whole forward (n_ops = all of them) and the
// prefixes alink_debug_vgg16_embed_prefix stops at are this one loop.  The arguments are already checked.
static int run_ops(alink_vgg16* r, const float* dev_in, int n, int preprocessed, float* dev_out, void* ws, size_t n_ops,
                   hipStream_t st) {
    const size_t one = ((size_t)n * r->buf_elems_per_image * 2 + 255) & ~(size_t)255;
    auto buf = [&](int id) -> void* { return (char*)ws + one * id; };
    const size_t nops = r->ops.size();
    for (size_t i = 0; i < n_ops; ++i) {
        const VOp& op = r->ops[i];
        if (op.kind == 0) {
            StemParams sp{};
            sp.in = dev_in; sp.wgt = r->d_stem_w; sp.bias = r->d_stem_bias; sp.alpha = r->d_zero_alpha; sp.out = buf(0);
            sp.N = n; sp.H = r->H; sp.W = r->W; sp.C0 = 64; sp.layout = ALINK_LAYOUT_NHWC_F32; sp.mul = 1.f;
            if (preprocessed) { sp.sub[0] = sp.sub[1] = sp.sub[2] = 0.f; sp.flip = 0; }
            else { sp.sub[0] = 93.5940f; sp.sub[1] = 104.7624f; sp.sub[2] = 129.1863f; sp.flip = 1; }
            ALINK_HIP(launch_stem(r->dtype, sp, st));
        } else if (op.kind == 1) {
            ConvParams p = op.cp;
            p.in = buf(op.in_buf); p.out = buf(op.out_buf); with_batch(p, n);
            ALINK_HIP(launch_conv(op.kernel, r->dtype, p, st));
        } else {
            const bool last = i + 1 == nops;
            const long long tot = (long long)n * (op.H / 2) * (op.W / 2) * (op.C / 8);
            const dim3 grid((unsigned)((tot + 255) / 256));
            if (r->dtype == ALINK_DT_BF16) {
                if (last) hipLaunchKernelGGL((maxpool2_kernel<__bf16, float>), grid, dim3(256), 0, st, (const __bf16*)buf(op.in_buf), dev_out, n, op.H, op.W, op.C);
                else      hipLaunchKernelGGL((maxpool2_kernel<__bf16, __bf16>), grid, dim3(256), 0, st, (const __bf16*)buf(op.in_buf), (__bf16*)buf(op.out_buf), n, op.H, op.W, op.C);
            } else {
                if (last) hipLaunchKernelGGL((maxpool2_kernel<_Float16, float>), grid, dim3(256), 0, st, (const _Float16*)buf(op.in_buf), dev_out, n, op.H, op.W, op.C);
                else      hipLaunchKernelGGL((maxpool2_kernel<_Float16, _Float16>), grid, dim3(256), 0, st, (const _Float16*)buf(op.in_buf), (_Float16*)buf(op.out_buf), n, op.H, op.W, op.C);
            }
        }
        ALINK_HIP(hipGetLastError());
    }
    return ALINK_OK;
}

// the argument checks of a forward over n images (after the handle's own); need_out: the last pool runs, which writes dev_out
static int check_forward_args(alink_vgg16* r, const float* dev_in, int n, const float* dev_out, bool need_out, const void* ws,
                              size_t ws_bytes) {
    ALINK_REQUIRE(dev_in && (dev_out || !need_out) && ws && n > 0, ALINK_EINVAL, "bad argument");
    ALINK_REQUIRE(((uintptr_t)ws & 255) == 0, ALINK_EINVAL, "workspace must be 256-byte aligned");
    ALINK_REQUIRE(ws_bytes >= alink_vgg16_workspace_bytes(r, n), ALINK_ENOMEM, "workspace too small");
    ALINK_REQUIRE((long long)n * r->buf_elems_per_image < (1ll << 31), ALINK_EINVAL, "batch of %d too large; split it", n);
    return ALINK_OK;
}

int alink_vgg16_embed(alink_vgg16_t* r, const float* dev_in, int n, int preprocessed, float* dev_out, void* ws,
                      size_t ws_bytes, void* stream) {
    ALINK_REQUIRE(r && r->finalized, ALINK_ESTATE, "alink_vgg16_embed before finalize");
    DeviceGuard dg(r->device);
    const int rc = check_forward_args(r, dev_in, n, dev_out, true, ws, ws_bytes);
    if (rc) return rc;
    return run_ops(r, dev_in, n, preprocessed, dev_out, ws, r->ops.size(), (hipStream_t)stream);
}

// diagnostic (include/alink_hip_debug.h): the forward stopped after its first n_ops ops, and where and what op n_ops - 1 wrote
int alink_debug_vgg16_embed_prefix(alink_vgg16_t* r, const float* dev_in, int n, int preprocessed, float* dev_out, void* ws,
                                   size_t ws_bytes, void* stream, int n_ops, size_t* byte_offset, int* H, int* W, int* C,
                                   char* name_buf, int name_len, int* kernel, int* form) {
    if (!r || !r->finalized) { set_error("alink_debug_vgg16_embed_prefix before finalize"); return -1; }
    const int nops = (int)r->ops.size();
    if (n_ops <= 0) return nops;
    if (n_ops > nops) { set_error("the network has %d ops, asked for %d", nops, n_ops); return -1; }
    DeviceGuard dg(r->device);
    if (check_forward_args(r, dev_in, n, dev_out, n_ops == nops, ws, ws_bytes)) return -1;
    const VOp& op = r->ops[n_ops - 1];
    const size_t one = ((size_t)n * r->buf_elems_per_image * 2 + 255) & ~(size_t)255;
    if (byte_offset) *byte_offset = n_ops == nops ? 0 : one * op.out_buf;
    if (H) *H = op.kind == 0 ? r->H : (op.kind == 1 ? op.cp.Ho : op.H / 2);
    if (W) *W = op.kind == 0 ? r->W : (op.kind == 1 ? op.cp.Wo : op.W / 2);
    if (C) *C = op.kind == 0 ? 64 : (op.kind == 1 ? op.cp.Cout : op.C);
    if (name_buf && name_len > 0) snprintf(name_buf, (size_t)name_len, "%s", op.name.c_str());
    if (kernel) *kernel = op.kind == 1 ? (int)op.kernel : -1;
    if (form) {
        *form = 0;
        if (op.kind == 1) {
            ConvParams p = op.cp;
            with_batch(p, n);
            *form = served_form(op.kernel, r->dtype, p);
        }
    }
    if (run_ops(r, dev_in, n, preprocessed, dev_out, ws, (size_t)n_ops, (hipStream_t)stream)) return -1;
    return nops;
}

}  // extern "C"
