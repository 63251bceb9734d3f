// convnet_kernels.h -- the ConvolutionalNet kernels, included by convnet.hip once per arithmetic: in namespace
// rsd::convnet_exact under the library's -ffp-contract=off (every multiply and add rounds on its own, in the
// reference's order) and in rsd::convnet_fast under `#pragma clang fp contract(fast)` (the same loops, the compiler
// may fuse a multiply and its add into one FMA; nothing else about the arithmetic changes, so the error bound of an
// n-term dot product holds).  RSD_CONVNET_NS names the namespace.
//
// Both kernels accumulate NCO output channels of one texel in registers: the input value of a tap is read once (from
// memory in the per-layer kernel, from LDS in the fused one) and meets NCO weights.  The weights of a slice are the
// same for every lane of a workgroup (the slice is blockIdx.z): they are read through a pointer built from kernel
// arguments and blockIdx alone, in the constant address space (no kernel writes the weights), which the compiler turns
// into scalar loads; the host stores them in the order the loops consume them, [term][CoutPad] with the terms in
// execution order (convnet.hip build_net), so a term's NCO weights are one contiguous scalar load.
namespace RSD_CONVNET_NS {

typedef const float __attribute__((address_space(4))) * ConvWeights;

template <int PREC>
__device__ __forceinline__ float load_act(const void* __restrict__ p, size_t i) {
    if (PREC == RSD_CONVNET_FLOAT) return reinterpret_cast<const float*>(p)[i];
    if (PREC == RSD_CONVNET_HALF) return __half2float(reinterpret_cast<const __half*>(p)[i]);
    return unorm8_to_float(reinterpret_cast<const uint8_t*>(p)[i]);
}

template <int PREC>
__device__ __forceinline__ void store_act(void* __restrict__ p, size_t i, float v) {
    if (PREC == RSD_CONVNET_FLOAT) reinterpret_cast<float*>(p)[i] = v;
    else if (PREC == RSD_CONVNET_HALF) reinterpret_cast<__half*>(p)[i] = __float2half_rn(v);
    else reinterpret_cast<uint8_t*>(p)[i] = unorm8(v);
}

// texel i of input channel c (bright, dark, importance, depth): R8Unorm or R32Float
__device__ __forceinline__ float load_input(const ConvInputs& in, int c, size_t i) {
    const void* p = c == 0 ? in.p0 : (c == 1 ? in.p1 : (c == 2 ? in.p2 : in.p3));
    const int bytes = c == 0 ? in.b0 : (c == 1 ? in.b1 : (c == 2 ? in.b2 : in.b3));
    return bytes == 1 ? unorm8_to_float(reinterpret_cast<const uint8_t*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// the last layer's activation (ConvolutionNet.h:218-224): HLSL clamp(v, dark, bright) = min(max(v, dark), bright)
__device__ __forceinline__ float final_value(const ConvInputs& in, int clampOut, float v, size_t i) {
    if (!clampOut) return v;
    return fminf(fmaxf(v, load_input(in, 1, i)), load_input(in, 0, i));
}

// ---- one launch per layer: blocks of 64 x 4 texels of the scissor rectangle, blockIdx.z the slice
template <int PREC, int NCO, bool FIRST>
__global__ void __launch_bounds__(kConvLayerW* kConvLayerH) convnet_layer_kernel(ConvLayerArgs a,
                                                                                 const float* __restrict__ weights) {
    const int x = a.g + (int)(blockIdx.x * kConvLayerW + threadIdx.x);
    const int y = a.g + (int)(blockIdx.y * kConvLayerH + threadIdx.y);
    const int s = (int)blockIdx.z;
    if (x >= a.qw - a.g || y >= a.qh - a.g) return;
    const ConvLayerDesc d = a.net.layer[a.l];
    constexpr int G = FIRST ? 1 : 4;  // input channels per texture fetch of the reference (ConvolutionNet.h:160-161)
    const int K = d.K, lo = d.K / 2, Cin = d.Cin;
    const size_t plane = (size_t)a.qw * a.qh, centre = (size_t)y * a.qw + x;
    ConvWeights wb = (ConvWeights)weights + (size_t)s * a.net.sliceStride + d.wOff;
    for (int co0 = 0; co0 < a.coutUsed; co0 += NCO) {
        float acc[NCO];
#pragma unroll
        for (int j = 0; j < NCO; ++j) acc[j] = wb[co0 + j];
        ConvWeights w = wb + d.CoutPad + co0;
        for (int c0 = 0; c0 < Cin; c0 += G)
            for (int b = 0; b < K; ++b)
                for (int ka = 0; ka < K; ++ka) {
                    const int xx = x + ka - lo, yy = y + b - lo;
                    // the first layer reads the inputs wherever the image has them, the others the previous layer,
                    // which exists inside the scissor only
                    const bool ok = FIRST ? (xx >= 0 && xx < a.qw && yy >= 0 && yy < a.qh)
                                          : (xx >= a.g && xx < a.qw - a.g && yy >= a.g && yy < a.qh - a.g);
                    const size_t t = (size_t)yy * a.qw + xx;
#pragma unroll
                    for (int sub = 0; sub < G; ++sub) {
                        const int c = c0 + sub;
                        if (c >= Cin) break;
                        float v = 0.0f;
                        if (ok) v = FIRST ? load_input(a.in, c, (size_t)s * plane + t)
                                          : load_act<PREC>(a.src, ((size_t)s * Cin + c) * plane + t);
#pragma unroll
                        for (int j = 0; j < NCO; ++j) acc[j] += v * w[j];
                        w += d.CoutPad;
                    }
                }
#pragma unroll
        for (int j = 0; j < NCO; ++j) {
            const int co = co0 + j;
            if (co >= a.coutUsed) break;
            if (a.last) a.out[(size_t)s * plane + centre] = final_value(a.in, a.clampOut, acc[j], (size_t)s * plane + centre);
            else store_act<PREC>(a.dst, ((size_t)s * d.Cout + co) * plane + centre, fmaxf(0.0f, acc[j]));
        }
    }
}

// ---- the whole net in one launch (Float precision): a workgroup owns a kConvTileW x kConvTileH output tile of one
// slice.  LDS holds two buffers; the input tile with the net's full halo goes into A, layer 0 writes the
// activations of the region its successors still need into B, layer 1 back into A, ...; the last layer writes
// channel 0 of the tile to memory.  A region texel outside the scissor holds 0 (it is never drawn).
template <int NCO, int G>
__device__ __forceinline__ void fused_layer(const ConvFusedArgs& a, const ConvLayerDesc& d, bool last, int coutUsed,
                                            ConvWeights wb, const float* __restrict__ src, int srcW,
                                            int srcArea, float* __restrict__ dst, int rw, int rh, int x0, int y0,
                                            size_t sliceBase) {
    const int area = rw * rh, K = d.K, Cin = d.Cin;
    for (int i = (int)threadIdx.x; i < area; i += kConvFusedThreads) {
        const int ry = i / rw, rx = i - ry * rw;
        const int gx = x0 + rx, gy = y0 + ry;
        if (!(gx >= a.g && gx < a.qw - a.g && gy >= a.g && gy < a.qh - a.g)) {
            if (!last)
                for (int co = 0; co < d.Cout; ++co) dst[co * area + i] = 0.0f;
            continue;
        }
        for (int co0 = 0; co0 < coutUsed; co0 += NCO) {
            float acc[NCO];
#pragma unroll
            for (int j = 0; j < NCO; ++j) acc[j] = wb[co0 + j];
            ConvWeights w = wb + d.CoutPad + co0;
            for (int c0 = 0; c0 < Cin; c0 += G)
                for (int b = 0; b < K; ++b)
                    for (int ka = 0; ka < K; ++ka) {
                        // region texel (rx, ry) of this layer is texel (rx + lo, ry + lo) of the source region
                        const int t = (ry + b) * srcW + rx + ka;
#pragma unroll
                        for (int sub = 0; sub < G; ++sub) {
                            const int c = c0 + sub;
                            if (c >= Cin) break;
                            const float v = src[c * srcArea + t];
#pragma unroll
                            for (int j = 0; j < NCO; ++j) acc[j] += v * w[j];
                            w += d.CoutPad;
                        }
                    }
#pragma unroll
            for (int j = 0; j < NCO; ++j) {
                const int co = co0 + j;
                if (co >= coutUsed) break;
                if (last) {
                    const size_t o = sliceBase + (size_t)gy * a.qw + gx;
                    a.out[o] = final_value(a.in, a.clampOut, acc[j], o);
                } else {
                    dst[co * area + i] = fmaxf(0.0f, acc[j]);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kConvFusedThreads) convnet_fused_kernel(ConvFusedArgs a,
                                                                             const float* __restrict__ weights) {
    extern __shared__ float convnet_lds[];
    float* bufA = convnet_lds;
    float* bufB = convnet_lds + a.bufAFloats;
    const int tx0 = a.g + (int)blockIdx.x * kConvTileW, ty0 = a.g + (int)blockIdx.y * kConvTileH;
    const int s = (int)blockIdx.z;
    const size_t sliceBase = (size_t)s * a.qw * a.qh;
    int lo = a.loAll, hi = a.hiAll;  // how far the region of this stage reaches beyond the tile, towards -/+
    int rw = kConvTileW + lo + hi, rh = kConvTileH + lo + hi;
    {
        const int area = rw * rh, Cin0 = a.net.layer[0].Cin;
        for (int c = 0; c < Cin0; ++c)
            for (int i = (int)threadIdx.x; i < area; i += kConvFusedThreads) {
                const int ry = i / rw, rx = i - ry * rw;
                const int gx = tx0 - lo + rx, gy = ty0 - lo + ry;
                float v = 0.0f;  // a tap outside the image reads 0
                if (gx >= 0 && gx < a.qw && gy >= 0 && gy < a.qh) v = load_input(a.in, c, sliceBase + (size_t)gy * a.qw + gx);
                bufA[c * area + i] = v;
            }
    }
    __syncthreads();
    const float* src = bufA;
    float* dst = bufB;
    for (int l = 0; l < a.net.L; ++l) {
        const ConvLayerDesc d = a.net.layer[l];
        const int srcW = rw, srcArea = rw * rh;
        lo -= d.K / 2;
        hi -= d.K - 1 - d.K / 2;
        rw = kConvTileW + lo + hi;
        rh = kConvTileH + lo + hi;
        const bool last = l == a.net.L - 1;
        const int coutUsed = last ? 1 : d.Cout;
        ConvWeights wb = (ConvWeights)weights + (size_t)s * a.net.sliceStride + d.wOff;
        const int x0 = tx0 - lo, y0 = ty0 - lo;
        if (l == 0) {
            if (d.nco == 8) fused_layer<8, 1>(a, d, last, coutUsed, wb, src, srcW, srcArea, dst, rw, rh, x0, y0, sliceBase);
            else if (d.nco == 4) fused_layer<4, 1>(a, d, last, coutUsed, wb, src, srcW, srcArea, dst, rw, rh, x0, y0, sliceBase);
            else fused_layer<1, 1>(a, d, last, coutUsed, wb, src, srcW, srcArea, dst, rw, rh, x0, y0, sliceBase);
        } else {
            if (d.nco == 8) fused_layer<8, 4>(a, d, last, coutUsed, wb, src, srcW, srcArea, dst, rw, rh, x0, y0, sliceBase);
            else if (d.nco == 4) fused_layer<4, 4>(a, d, last, coutUsed, wb, src, srcW, srcArea, dst, rw, rh, x0, y0, sliceBase);
            else fused_layer<1, 4>(a, d, last, coutUsed, wb, src, srcW, srcArea, dst, rw, rh, x0, y0, sliceBase);
        }
        __syncthreads();
        const float* t = src;
        src = dst;
        dst = const_cast<float*>(t);
    }
}

}  // namespace RSD_CONVNET_NS
