// convnet.hip -- the ConvolutionalNet pass of the reference (RenderPasses/ConvolutionalNet: ConvolutionNet.h:115-231
// generates one pixel shader per layer and slice, ConvolutionalNet.cpp:131-235 draws them): the learned resolve of
// the (bright, dark) AO pair.  A small convolutional net per array slice reads bright, dark, importance and depth
// (channels 0..3), applies ReLU between the layers and clamps channel 0 of the last layer into [dark, bright].
//
// What the reference fixes, and this file keeps:
//   - weight axis order: the .npy array is [A][B][Cin][Cout] and Matrix::get strides kx over axis 0, so w[a][b]
//     applies at (x + a - K/2, y + b - K/2): axis 0 is the x offset, the transpose of the Keras layout;
//   - a tap outside the image reads 0 (Texture operator[] out of range);
//   - the order of the sum: o = bias, then input channel (the first layer) or group of four channels (the packed
//     RGBA intermediates of the others), then y, then x, then the channel within the group; padded channels are
//     skipped;
//   - the scissor guardBand / 4 of every draw (setGuardBandScissors, :159): the intermediates outside it are never
//     written -- they read 0 here, a freshly created texture's content -- and the output keeps its old value;
//   - the formats of the intermediates: float, half or unorm (getMatchingLayerOutputFormat).
// The reference draws layers x slices full-screen passes; here one launch per layer covers all slices, or one launch
// runs the whole net out of LDS (convnet_kernels.h).  The net object is host memory until the first run on a device.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsd_graph.h"
#include "host/npy.h"
#include "rsd_device.h"
#include "rsd_internal.h"

namespace rsd {

constexpr int kConvMaxLayers = 8, kConvMaxKernel = 7, kConvMaxChannels = 32;
constexpr int kConvLayerW = 64, kConvLayerH = 4;  // per-layer kernel: post.hip's block shape
// fused kernel: 256 threads own a 32 x 16 output tile, two texels each in the last layer
constexpr int kConvTileW = 32, kConvTileH = 16, kConvFusedThreads = 256;
// LDS one workgroup of the fused kernel may take: at most two fit the 160 KiB of a CU
constexpr size_t kConvFusedLdsMax = 64 * 1024;

struct ConvLayerDesc {
    int K, Cin, Cout;
    int CoutPad;  // Cout rounded up to 4: the stride of a term's weights
    int nco;      // output channels accumulated at once: 8, 4, or 1 for the last layer (only channel 0 is output)
    int wOff;     // floats from the slice's block to this layer's bias [CoutPad]; the weights follow
};
struct ConvNetDesc {
    int L;
    int sliceStride;  // floats per slice
    ConvLayerDesc layer[kConvMaxLayers];
};
struct ConvInputs {
    const void *p0, *p1, *p2, *p3;
    int b0, b1, b2, b3;  // bytes per texel
};
struct ConvLayerArgs {
    ConvNetDesc net;
    ConvInputs in;
    const void* src;  // the previous layer's activations, [slice][Cin][qh][qw]
    void* dst;        // this layer's
    float* out;
    int l, last, coutUsed, clampOut;
    int qw, qh, g;
};
struct ConvFusedArgs {
    ConvNetDesc net;
    ConvInputs in;
    float* out;
    int clampOut, qw, qh, g;
    int loAll, hiAll;  // the net's reach towards -x / -y and towards +x / +y
    int bufAFloats;
};

}  // namespace rsd

#define RSD_CONVNET_NS convnet_exact
namespace rsd {
#include "convnet_kernels.h"
}
#undef RSD_CONVNET_NS
#define RSD_CONVNET_NS convnet_fast
#pragma clang fp contract(fast)
namespace rsd {
#include "convnet_kernels.h"
}
#pragma clang fp contract(off)
#undef RSD_CONVNET_NS

struct rsd_convnet {
    uint32_t L = 0, S = 0;
    uint32_t K[rsd::kConvMaxLayers] = {}, Cin[rsd::kConvMaxLayers] = {}, Cout[rsd::kConvMaxLayers] = {};
    rsd::ConvNetDesc desc{};
    std::vector<float> packed;  // [slice][layer: bias[CoutPad], weights[term][CoutPad]]
    uint32_t radius = 0, loAll = 0, hiAll = 0;
    bool fused = false;
    size_t bufAFloats = 0, ldsBytes = 0;
    std::mutex mutex;
    std::vector<std::pair<int, float*>> uploaded;  // (HIP device, weights)
};

namespace rsd {
namespace {

float round_like_the_shader_text(float w) {  // operator<<(float): 6 significant digits, "%g"
    char text[64];
    std::snprintf(text, sizeof text, "%g", (double)w);
    return (float)std::strtod(text, nullptr);
}

// Validates the shapes, packs the weights in execution order and sizes the fused kernel's LDS.
// weights[l]: [S][K][K][Cin][Cout], bias[l]: [S][Cout] or null.
rsd_status build_net(const rsd_convnet_layer* layers, uint32_t L, uint32_t S, const char* who, rsd_convnet** out) {
    if (L < 1 || L > (uint32_t)kConvMaxLayers) {
        set_error(std::string(who) + ": a net has 1..8 layers");
        return RSD_ERR_UNSUPPORTED;
    }
    if (S != 1 && S != 16) {
        set_error(std::string(who) + ": slices must be 1 (a plain image) or 16 (a deinterleaved one)");
        return RSD_ERR_UNSUPPORTED;
    }
    for (uint32_t l = 0; l < L; ++l) {
        const rsd_convnet_layer& y = layers[l];
        if (!y.weights) {
            set_error(std::string(who) + ": invalid argument (null weights)");
            return RSD_ERR_INVALID_ARG;
        }
        if (y.kernel < 1 || y.kernel > (uint32_t)kConvMaxKernel || y.channels_in < 1 || y.channels_out < 1 ||
            y.channels_in > (uint32_t)kConvMaxChannels || y.channels_out > (uint32_t)kConvMaxChannels) {
            set_error(std::string(who) + ": layer " + std::to_string(l) + ": kernel must be 1..7 and the channel counts 1..32");
            return RSD_ERR_UNSUPPORTED;
        }
        if (l == 0 && y.channels_in > 4) {
            set_error(std::string(who) + ": the first layer reads at most 4 channels (bright, dark, importance, depth)");
            return RSD_ERR_UNSUPPORTED;
        }
        if (l > 0 && y.channels_in != layers[l - 1].channels_out) {
            set_error(std::string(who) + ": layer " + std::to_string(l) + " reads " + std::to_string(y.channels_in) +
                      " channels, layer " + std::to_string(l - 1) + " writes " + std::to_string(layers[l - 1].channels_out));
            return RSD_ERR_UNSUPPORTED;
        }
    }
    auto* n = new rsd_convnet;
    n->L = L;
    n->S = S;
    int off = 0;
    for (uint32_t l = 0; l < L; ++l) {
        ConvLayerDesc& d = n->desc.layer[l];
        n->K[l] = layers[l].kernel;
        n->Cin[l] = layers[l].channels_in;
        n->Cout[l] = layers[l].channels_out;
        d.K = (int)n->K[l];
        d.Cin = (int)n->Cin[l];
        d.Cout = (int)n->Cout[l];
        d.CoutPad = (d.Cout + 3) / 4 * 4;
        d.nco = l == L - 1 ? 1 : (d.CoutPad % 8 == 0 ? 8 : 4);
        d.wOff = off;
        off += d.CoutPad * (1 + d.K * d.K * d.Cin);
        n->loAll += (uint32_t)(d.K / 2);
        n->hiAll += (uint32_t)(d.K - 1 - d.K / 2);
    }
    n->radius = n->loAll;
    n->desc.L = (int)L;
    n->desc.sliceStride = off;
    n->packed.assign((size_t)off * S, 0.0f);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t l = 0; l < L; ++l) {
            const ConvLayerDesc& d = n->desc.layer[l];
            float* bias = n->packed.data() + (size_t)s * off + d.wOff;
            float* w = bias + d.CoutPad;
            if (layers[l].bias)
                for (int co = 0; co < d.Cout; ++co) bias[co] = layers[l].bias[(size_t)s * d.Cout + co];
            const float* src = layers[l].weights + (size_t)s * d.K * d.K * d.Cin * d.Cout;
            const int G = l == 0 ? 1 : 4;
            size_t term = 0;
            for (int c0 = 0; c0 < d.Cin; c0 += G)
                for (int b = 0; b < d.K; ++b)
                    for (int a = 0; a < d.K; ++a)
                        for (int sub = 0; sub < G && c0 + sub < d.Cin; ++sub, ++term)
                            for (int co = 0; co < d.Cout; ++co)
                                w[term * d.CoutPad + co] = src[(((size_t)a * d.K + b) * d.Cin + (c0 + sub)) * d.Cout + co];
        }
    // LDS of the fused kernel: the input region in A, layer 0 into B, layer 1 into A, ...; the last layer writes memory
    size_t bufA = 0, bufB = 0;
    int lo = (int)n->loAll, hi = (int)n->hiAll;
    bufA = (size_t)n->Cin[0] * (kConvTileW + lo + hi) * (kConvTileH + lo + hi);
    for (uint32_t l = 0; l + 1 < L; ++l) {
        lo -= (int)n->K[l] / 2;
        hi -= (int)n->K[l] - 1 - (int)n->K[l] / 2;
        const size_t need = (size_t)n->Cout[l] * (kConvTileW + lo + hi) * (kConvTileH + lo + hi);
        size_t& buf = l % 2 == 0 ? bufB : bufA;
        if (need > buf) buf = need;
    }
    n->bufAFloats = bufA;
    n->ldsBytes = (bufA + bufB) * sizeof(float);
    n->fused = n->ldsBytes <= kConvFusedLdsMax;
    *out = n;
    return RSD_OK;
}

struct ConvRect {
    int qw, qh, g;
    bool empty;
};
ConvRect conv_rect(const rsd_convnet_params* p) {
    ConvRect r{};
    r.qw = (int)(p->layers == 16 ? (p->width + 3) / 4 : p->width);
    r.qh = (int)(p->layers == 16 ? (p->height + 3) / 4 : p->height);
    // setGuardBandScissors(quarterRes, guardBand / 4) (ConvolutionalNet.cpp:147-159), rsd_ao_guided_blur's rule
    r.g = (int)(p->layers > 1 ? p->guard_band / (uint32_t)(int)(std::sqrt((double)p->layers) + 0.5) : p->guard_band);
    r.empty = 2 * (int64_t)r.g >= r.qw || 2 * (int64_t)r.g >= r.qh;
    return r;
}

size_t precision_bytes(uint32_t precision) { return precision == RSD_CONVNET_FLOAT ? 4 : (precision == RSD_CONVNET_HALF ? 2 : 1); }

// byte offsets of the layers' activations in d_scratch; returns the total
uint64_t scratch_layout(const rsd_convnet* n, const rsd_convnet_params* p, uint64_t offs[kConvMaxLayers]) {
    const ConvRect r = conv_rect(p);
    uint64_t total = 0;
    for (uint32_t l = 0; l + 1 < n->L; ++l) {
        offs[l] = total;
        const uint64_t bytes = (uint64_t)n->S * n->Cout[l] * (uint64_t)r.qw * r.qh * precision_bytes(p->precision);
        total += (bytes + 255) / 256 * 256;
    }
    return total;
}

rsd_status device_weights(rsd_convnet* n, const float** out) {
    int dev = 0;
    RSD_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(n->mutex);
    for (auto& u : n->uploaded)
        if (u.first == dev) {
            *out = u.second;
            return RSD_OK;
        }
    float* d = nullptr;
    RSD_HIP(hipMalloc(&d, n->packed.size() * sizeof(float)));
    hipError_t e = hipMemcpy(d, n->packed.data(), n->packed.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "rsd_convnet_run: weight upload");
    }
    n->uploaded.emplace_back(dev, d);
    *out = d;
    return RSD_OK;
}

template <int PREC, bool FAST>
void launch_layer(const ConvLayerArgs& a, const float* w, int nco, uint32_t S, hipStream_t s) {
    const dim3 grid((uint32_t)(a.qw - 2 * a.g + kConvLayerW - 1) / kConvLayerW,
                    (uint32_t)(a.qh - 2 * a.g + kConvLayerH - 1) / kConvLayerH, S);
    const dim3 block(kConvLayerW, kConvLayerH);
#define RSD_CONV_LAUNCH(NS)                                                                                       \
    do {                                                                                                          \
        if (a.l == 0) {                                                                                           \
            if (nco == 8) hipLaunchKernelGGL((NS::convnet_layer_kernel<PREC, 8, true>), grid, block, 0, s, a, w);    \
            else if (nco == 4) hipLaunchKernelGGL((NS::convnet_layer_kernel<PREC, 4, true>), grid, block, 0, s, a, w); \
            else hipLaunchKernelGGL((NS::convnet_layer_kernel<PREC, 1, true>), grid, block, 0, s, a, w);             \
        } else {                                                                                                  \
            if (nco == 8) hipLaunchKernelGGL((NS::convnet_layer_kernel<PREC, 8, false>), grid, block, 0, s, a, w);   \
            else if (nco == 4) hipLaunchKernelGGL((NS::convnet_layer_kernel<PREC, 4, false>), grid, block, 0, s, a, w); \
            else hipLaunchKernelGGL((NS::convnet_layer_kernel<PREC, 1, false>), grid, block, 0, s, a, w);            \
        }                                                                                                         \
    } while (0)
    if constexpr (FAST) RSD_CONV_LAUNCH(convnet_fast);
    else RSD_CONV_LAUNCH(convnet_exact);
#undef RSD_CONV_LAUNCH
}

}  // namespace
}  // namespace rsd

using namespace rsd;

extern "C" rsd_status rsd_convnet_create(const rsd_convnet_layer* layers, uint32_t layer_count, uint32_t slices,
                                         rsd_convnet** out) {
    if (!layers || !out) {
        set_error("rsd_convnet_create: invalid argument (null pointer)");
        return RSD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    return build_net(layers, layer_count, slices, "rsd_convnet_create", out);
}

extern "C" rsd_status rsd_convnet_load_dir(const char* dir, uint32_t slices, rsd_convnet** out) {
    if (!dir || !out) {
        set_error("rsd_convnet_load_dir: invalid argument (null pointer)");
        return RSD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (slices != 1 && slices != 16) {
        set_error("rsd_convnet_load_dir: slices must be 1 (a plain image) or 16 (a deinterleaved one)");
        return RSD_ERR_UNSUPPORTED;
    }
    const std::string base = std::string(dir) + "/";
    auto exists = [](const std::string& path) {
        FILE* f = std::fopen(path.c_str(), "rb");
        if (f) std::fclose(f);
        return f != nullptr;
    };
    // slice 0 decides the shape of the net; every other slice must match it (the reference sizes every slice's
    // intermediates from slice 0, ConvolutionalNet.cpp:99-108)
    std::vector<std::vector<float>> weights, bias;  // per layer, all slices
    std::vector<rsd_convnet_layer> layers;
    std::string err;
    for (uint32_t s = 0; s < slices; ++s) {
        uint32_t l = 0;
        for (;; ++l) {
            const std::string wname = base + std::to_string(s) + "_weight_" + std::to_string(l) + ".npy";
            const std::string bname = base + std::to_string(s) + "_bias_" + std::to_string(l) + ".npy";
            if (!exists(wname)) break;
            npy::Array w;
            if (!npy::load(wname, w, err)) {
                set_error("rsd_convnet_load_dir: " + err);
                return RSD_ERR_INVALID_ARG;
            }
            if (w.shape.size() != 4) {
                set_error("rsd_convnet_load_dir: " + wname + ": weights must be a 4-d array [K][K][Cin][Cout]");
                return RSD_ERR_INVALID_ARG;
            }
            if (w.shape[0] != w.shape[1]) {
                set_error("rsd_convnet_load_dir: " + wname + ": non-square kernels are not supported");
                return RSD_ERR_UNSUPPORTED;
            }
            if (w.shape[0] > (uint64_t)kConvMaxKernel || w.shape[2] > (uint64_t)kConvMaxChannels ||
                w.shape[3] > (uint64_t)kConvMaxChannels || w.data.empty()) {
                set_error("rsd_convnet_load_dir: " + wname + ": kernel must be 1..7 and the channel counts 1..32");
                return RSD_ERR_UNSUPPORTED;
            }
            if (s == 0) {
                if (l >= (uint32_t)kConvMaxLayers) {
                    set_error("rsd_convnet_load_dir: a net has 1..8 layers");
                    return RSD_ERR_UNSUPPORTED;
                }
                layers.push_back({(uint32_t)w.shape[0], (uint32_t)w.shape[2], (uint32_t)w.shape[3], nullptr, nullptr});
                weights.emplace_back();
                bias.emplace_back();
            } else if (l >= layers.size() || layers[l].kernel != w.shape[0] || layers[l].channels_in != w.shape[2] ||
                       layers[l].channels_out != w.shape[3]) {
                set_error("rsd_convnet_load_dir: " + wname + ": every slice must have the layers, kernel sizes and channel counts of slice 0");
                return RSD_ERR_UNSUPPORTED;
            }
            weights[l].insert(weights[l].end(), w.data.begin(), w.data.end());
            std::vector<float> b((size_t)layers[l].channels_out, 0.0f);  // a missing bias file: zeros (ConvolutionNet.h:91-99)
            if (exists(bname)) {
                npy::Array ba;
                if (!npy::load(bname, ba, err)) {
                    set_error("rsd_convnet_load_dir: " + err);
                    return RSD_ERR_INVALID_ARG;
                }
                if (ba.shape.size() != 1 || ba.shape[0] != layers[l].channels_out) {
                    set_error("rsd_convnet_load_dir: " + bname + ": the bias must be a 1-d array of the layer's output channels");
                    return RSD_ERR_INVALID_ARG;
                }
                b = ba.data;
            }
            bias[l].insert(bias[l].end(), b.begin(), b.end());
        }
        if (s == 0 && l == 0) {
            set_error("rsd_convnet_load_dir: no network in " + std::string(dir) + " (no 0_weight_0.npy)");
            return RSD_ERR_INVALID_ARG;
        }
        if (l != layers.size()) {
            set_error("rsd_convnet_load_dir: slice " + std::to_string(s) + " has " + std::to_string(l) + " layers, slice 0 has " +
                      std::to_string(layers.size()) + " (mismatching layer count)");
            return RSD_ERR_UNSUPPORTED;
        }
    }
    for (size_t l = 0; l < layers.size(); ++l) {
        for (float& v : weights[l]) v = round_like_the_shader_text(v);
        for (float& v : bias[l]) v = round_like_the_shader_text(v);
        layers[l].weights = weights[l].data();
        layers[l].bias = bias[l].data();
    }
    return build_net(layers.data(), (uint32_t)layers.size(), slices, "rsd_convnet_load_dir", out);
}

extern "C" void rsd_convnet_release(rsd_convnet* net) {
    if (!net) return;
    for (auto& u : net->uploaded) (void)hipFree(u.second);
    delete net;
}

extern "C" rsd_status rsd_convnet_get_info(const rsd_convnet* net, rsd_convnet_info* info) {
    if (!net || !info) {
        set_error("rsd_convnet_get_info: invalid argument (null pointer)");
        return RSD_ERR_INVALID_ARG;
    }
    std::memset(info, 0, sizeof *info);
    info->layers = net->L;
    info->slices = net->S;
    info->radius = net->radius;
    info->fused = net->fused ? 1u : 0u;
    for (uint32_t l = 0; l < net->L; ++l) {
        info->kernel[l] = net->K[l];
        info->channels_in[l] = net->Cin[l];
        info->channels_out[l] = net->Cout[l];
    }
    return RSD_OK;
}

extern "C" uint64_t rsd_convnet_scratch_bytes(const rsd_convnet* net, const rsd_convnet_params* params) {
    if (!net || !params || params->precision > RSD_CONVNET_UNORM || (params->layers != 1 && params->layers != 16))
        return 0;
    uint64_t offs[kConvMaxLayers];
    return scratch_layout(net, params, offs);
}

extern "C" rsd_status rsd_convnet_run(rsd_convnet* net, const rsd_convnet_params* params, const void* d_bright,
                                      const void* d_dark, const void* d_importance, const void* d_depth,
                                      void* d_scratch, float* d_out, rsd_stream stream) {
    if (!net || !params || !d_out) {
        set_error("rsd_convnet_run: invalid argument (null pointer)");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->width == 0 || params->height == 0) {
        set_error("rsd_convnet_run: invalid argument (empty extent)");
        return RSD_ERR_INVALID_ARG;
    }
    const void* inputs[4] = {d_bright, d_dark, d_importance, d_depth};
    for (uint32_t c = 0; c < 4; ++c) {
        const bool needed = c < net->Cin[0] || (c < 2 && params->clamp_output);
        if (needed && !inputs[c]) {
            set_error("rsd_convnet_run: invalid argument (null input the net or the clamp reads)");
            return RSD_ERR_INVALID_ARG;
        }
        if (params->in_texel_bytes[c] != 1 && params->in_texel_bytes[c] != 4) {
            set_error("rsd_convnet_run: in_texel_bytes must be 1 (R8Unorm) or 4 (R32Float)");
            return RSD_ERR_INVALID_ARG;
        }
    }
    if (params->numerics > RSD_NUMERICS_EXACT) {
        set_error("rsd_convnet_run: numerics must be RSD_NUMERICS_FAST or RSD_NUMERICS_EXACT");
        return RSD_ERR_INVALID_ARG;
    }
    if (params->layers != net->S) {
        set_error("rsd_convnet_run: layers must equal the net's slices (" + std::to_string(net->S) + ")");
        return RSD_ERR_UNSUPPORTED;
    }
    if (params->precision > RSD_CONVNET_UNORM) {
        set_error("rsd_convnet_run: precision must be Float (0), Half (1) or UNorm (2)");
        return RSD_ERR_UNSUPPORTED;
    }
    uint64_t offs[kConvMaxLayers] = {};
    const uint64_t scratchBytes = scratch_layout(net, params, offs);
    if (scratchBytes != 0 && !d_scratch) {
        set_error("rsd_convnet_run: invalid argument (null scratch)");
        return RSD_ERR_INVALID_ARG;
    }
    const ConvRect r = conv_rect(params);
    if ((uint64_t)net->S * kConvMaxChannels * (uint64_t)r.qw * r.qh > 0x7fffffffull) {
        set_error("rsd_convnet_run: the image is too large");
        return RSD_ERR_UNSUPPORTED;
    }
    if (r.empty) return RSD_OK;  // an empty scissor: nothing is drawn

    // Half and UNorm intermediates always take the exact arithmetic
    const bool fast = params->numerics == RSD_NUMERICS_FAST && params->precision == RSD_CONVNET_FLOAT;
    const char* env = std::getenv("RSD_CONVNET_FUSED");
    const bool fused = net->fused && params->precision == RSD_CONVNET_FLOAT && !(env && std::strcmp(env, "off") == 0);
    const float* d_weights = nullptr;
    rsd_status st = device_weights(net, &d_weights);
    if (st != RSD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const ConvInputs in{d_bright,
                        d_dark,
                        d_importance,
                        d_depth,
                        (int)params->in_texel_bytes[0],
                        (int)params->in_texel_bytes[1],
                        (int)params->in_texel_bytes[2],
                        (int)params->in_texel_bytes[3]};
    if (fused) {
        ConvFusedArgs a{};
        a.net = net->desc;
        a.in = in;
        a.out = d_out;
        a.clampOut = params->clamp_output ? 1 : 0;
        a.qw = r.qw;
        a.qh = r.qh;
        a.g = r.g;
        a.loAll = (int)net->loAll;
        a.hiAll = (int)net->hiAll;
        a.bufAFloats = (int)net->bufAFloats;
        const dim3 grid((uint32_t)(r.qw - 2 * r.g + kConvTileW - 1) / kConvTileW,
                        (uint32_t)(r.qh - 2 * r.g + kConvTileH - 1) / kConvTileH, net->S);
        if (fast) hipLaunchKernelGGL(convnet_fast::convnet_fused_kernel, grid, dim3(kConvFusedThreads), net->ldsBytes, s, a, d_weights);
        else hipLaunchKernelGGL(convnet_exact::convnet_fused_kernel, grid, dim3(kConvFusedThreads), net->ldsBytes, s, a, d_weights);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? RSD_OK : hip_fail(e, "convnet_fused_kernel launch");
    }
    for (uint32_t l = 0; l < net->L; ++l) {
        ConvLayerArgs a{};
        a.net = net->desc;
        a.in = in;
        a.src = l > 0 ? (const uint8_t*)d_scratch + offs[l - 1] : nullptr;
        a.dst = l + 1 < net->L ? (uint8_t*)d_scratch + offs[l] : nullptr;
        a.out = d_out;
        a.l = (int)l;
        a.last = l + 1 == net->L;
        a.coutUsed = a.last ? 1 : (int)net->Cout[l];
        a.clampOut = params->clamp_output ? 1 : 0;
        a.qw = r.qw;
        a.qh = r.qh;
        a.g = r.g;
        const int nco = net->desc.layer[l].nco;
        if (fast) launch_layer<RSD_CONVNET_FLOAT, true>(a, d_weights, nco, net->S, s);
        else if (params->precision == RSD_CONVNET_FLOAT) launch_layer<RSD_CONVNET_FLOAT, false>(a, d_weights, nco, net->S, s);
        else if (params->precision == RSD_CONVNET_HALF) launch_layer<RSD_CONVNET_HALF, false>(a, d_weights, nco, net->S, s);
        else launch_layer<RSD_CONVNET_UNORM, false>(a, d_weights, nco, net->S, s);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "convnet_layer_kernel launch");
    }
    return RSD_OK;
}
