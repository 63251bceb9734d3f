// sd_walk_raster.hip -- walk 4 of the SD trace: the K nearest keys of every live ray from the triangles' side, then
// sd_row.h's resolve kernel over them.  (Overview: sd_common.h)
#include "sd_launch.h"
#include "sd_row.h"

namespace rsd {

// ------------------------------------------------------------------------------------
// Raster walk (RSD_WALK_RASTER).  Every SD ray starts at the camera position, so the canonical
// any-hit set of a texel -- the triangles its ray hits with TMin <= t <= TMax, culling applied --
// can be found from the triangles' side: project each triangle onto the SD texel grid (texel x's
// ray passes through image-plane x coordinate (sx + jitter) / dimx, jitter in (0, 1)), and run the
// exact watertight test (intersect_tri, the traversal's own) for the live texels under its
// footprint.  Hits go into the texel's K-list of 64-bit keys (t bits << 32 | prim: t > 0, so the
// integer order is the (t, prim) order) by the atomicMin insertion chain: the list ends with the K
// smallest keys whatever the insertion order, i.e. exactly the K nearest keys the BVH walks find,
// so sd_resolve_row_kernel<..., RASTER> gives the same bits.  The work is throughput-bound (one
// thread per triangle record, no dependent traversal chain): tiles whose live rays' view-depth
// range misses the triangle's are skipped, footprints over kRasterSmall texels are walked by the
// whole wave.
// ------------------------------------------------------------------------------------
constexpr int kRasterSmall = 16;

__device__ __forceinline__ float dot3(const float* a, f3 v) { return a[0] * v.x + a[1] * v.y + a[2] * v.z; }

// footprint of the triangle on the SD texel grid (clipped at the near plane wClip) and its view-
// depth range; false if it covers no texel of the map
__device__ __forceinline__ bool raster_footprint(const SDArgs& a, float4 v0, float4 v1, float4 v2, int& bx0, int& bx1,
                                                 int& by0, int& by1, float& zlo, float& zhi) {
    const rsd_camera& c = a.cam;
    const f3 o = mk(c.posW[0], c.posW[1], c.posW[2]);
    const f3 p[3] = {mk(v0.x - o.x, v0.y - o.y, v0.z - o.z), mk(v1.x - o.x, v1.y - o.y, v1.z - o.z),
                     mk(v2.x - o.x, v2.y - o.y, v2.z - o.z)};
    float pa[3], pb[3], pw[3];
    zlo = INFINITY;
    zhi = -INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pa[i] = dot3(a.projU, p[i]);
        pb[i] = dot3(a.projV, p[i]);
        pw[i] = dot3(a.projW, p[i]);
        const float z = dot3(a.camWn, p[i]);
        zlo = fminf(zlo, z);
        zhi = fmaxf(zhi, z);
    }
    // conservative depth range (float error of the dot products)
    const float zm = 1e-4f * fmaxf(fabsf(zlo), fabsf(zhi)) + 1e-4f;
    zlo -= zm;
    zhi += zm;
    const float wc = a.wClip;
    if (!(pw[0] >= wc || pw[1] >= wc || pw[2] >= wc)) return false;  // wholly behind the near clip
    float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = i == 2 ? 0 : i + 1;
        if (pw[i] >= wc) {
            const float u = pa[i] / pw[i], v = pb[i] / pw[i];
            xlo = fminf(xlo, u); xhi = fmaxf(xhi, u); ylo = fminf(ylo, v); yhi = fmaxf(yhi, v);
        }
        if ((pw[i] >= wc) != (pw[j] >= wc)) {  // the edge crosses the clip plane
            const float s = (wc - pw[i]) / (pw[j] - pw[i]);
            const float u = (pa[i] + s * (pa[j] - pa[i])) / wc, v = (pb[i] + s * (pb[j] - pb[i])) / wc;
            xlo = fminf(xlo, u); xhi = fmaxf(xhi, u); ylo = fminf(ylo, v); yhi = fmaxf(yhi, v);
        }
    }
    // NDC -> texel: sx + jitter = (ndcx + 1) / 2 * dimx, sy + jitter = (1 - ndcy) / 2 * dimy; 0.05 texel margin
    const int dimx = a.sdW - 2 * a.guard, dimy = a.sdH - 2 * a.guard;
    const float fx0 = (xlo + 1.0f) * 0.5f * (float)dimx - 0.05f, fx1 = (xhi + 1.0f) * 0.5f * (float)dimx + 0.05f;
    const float fy0 = (1.0f - yhi) * 0.5f * (float)dimy - 0.05f, fy1 = (1.0f - ylo) * 0.5f * (float)dimy + 0.05f;
    const float lim = 1e8f;  // near-clipped vertices project far away: clamp before converting
    bx0 = max((int)floorf(fmaxf(fx0, -lim)) + a.guard, 0);
    bx1 = min((int)floorf(fminf(fx1, lim)) + a.guard, a.sdW - 1);
    by0 = max((int)floorf(fmaxf(fy0, -lim)) + a.guard, 0);
    by1 = min((int)floorf(fminf(fy1, lim)) + a.guard, a.sdH - 1);
    return bx0 <= bx1 && by0 <= by1;
}

// may the live rays of 8x8 tile (tx, ty) hit a triangle of view depth [zlo, zhi]?  (false for tiles
// of other bands: their records may be stale)
__device__ __forceinline__ bool raster_tile(const SDArgs& a, int tx, int ty, float zlo, float zhi) {
    if (ty < a.bandStart || (ty - a.bandStart) % a.bandStep != 0 || (ty - a.bandStart) / a.bandStep >= a.bandN)
        return false;
    const float2 tr = a.tileRec[(size_t)ty * a.tilesW + tx];
    return zhi >= tr.x && zlo <= tr.y;  // a tile without live rays has the empty range [inf, -inf]
}

// one (triangle, texel) pair of a tile that passed raster_tile: slot, exact test, K-list insertion
template <int K>
__device__ __forceinline__ uint32_t raster_texel(const SDArgs& a, int x, int y, float4 v0, float4 v1, float4 v2,
                                                 const float4* __restrict__ queue) {
    const int32_t slot = a.slotMap[(size_t)y * a.sdW + x];
    if (slot < 0) return 0u;
    const float4 r0 = queue[2u * (uint32_t)slot], r1 = queue[2u * (uint32_t)slot + 1u];
    RayCtx r;
    ray_setup(r, mk(a.cam.posW[0], a.cam.posW[1], a.cam.posW[2]), mk(r0.x, r0.y, r0.z));
    float t, bu, bv, det;
    if (!intersect_tri(r, v0, v1, v2, t, bu, bv, det) || !(t >= r0.w && t <= r1.x) ||
        culled(det, __float_as_uint(v1.w), a.cull))
        return 1u;
    unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)__float_as_uint(v0.w);
    unsigned long long* L = a.keys64 + (size_t)slot * K;
    if (key >= __hip_atomic_load(&L[K - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 1u;
#pragma unroll
    for (int j = 0; j < K; ++j) {  // sorted insertion: each slot keeps the smaller key, the larger moves on
        const unsigned long long old = atomicMin(&L[j], key);
        if (old == ~0ull) break;
        key = old > key ? old : key;
    }
    return 1u;
}

template <int K>
__global__ void __launch_bounds__(kRasterBlock) sd_raster_kernel(SDArgs a, const float4* __restrict__ queue,
                                                                 const uint32_t* __restrict__ qctl) {
    const uint32_t i = blockIdx.x * kRasterBlock + threadIdx.x;
    const uint32_t liveCount = qctl[kQctlLiveTiles];
    const int lane = (int)(threadIdx.x & 63u);
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, v2 = v0;
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
    float zlo = 0.0f, zhi = 0.0f;
    bool any = false;
    if (i < a.nTris) {
        v0 = a.tris[3u * i];
        v1 = a.tris[3u * i + 1u];
        v2 = a.tris[3u * i + 2u];
        any = raster_footprint(a, v0, v1, v2, bx0, bx1, by0, by1, zlo, zhi);
    }
    const int area = any ? (bx1 - bx0 + 1) * (by1 - by0 + 1) : 0;
    uint32_t tests = 0u;
    if (any && area <= kRasterSmall)
        for (int y = by0; y <= by1; ++y)
            for (int x = bx0; x <= bx1; ++x)
                if (raster_tile(a, x >> 3, y >> 3, zlo, zhi)) tests += raster_texel<K>(a, x, y, v0, v1, v2, queue);
    // large footprints, one triangle at a time for the whole wave: the lanes test its 8x8 tiles,
    // then walk the texels of each passing tile (one lane per texel)
    for (unsigned long long bm = __ballot(area > kRasterSmall); bm; bm &= bm - 1ull) {
        const int b = __ffsll((long long)bm) - 1;
        const float4 w0 = make_float4(__shfl(v0.x, b), __shfl(v0.y, b), __shfl(v0.z, b), __shfl(v0.w, b));
        const float4 w1 = make_float4(__shfl(v1.x, b), __shfl(v1.y, b), __shfl(v1.z, b), __shfl(v1.w, b));
        const float4 w2 = make_float4(__shfl(v2.x, b), __shfl(v2.y, b), __shfl(v2.z, b), __shfl(v2.w, b));
        const int cx0 = __shfl(bx0, b), cx1 = __shfl(bx1, b), cy0 = __shfl(by0, b), cy1 = __shfl(by1, b);
        const float czlo = __shfl(zlo, b), czhi = __shfl(zhi, b);
        const int tx0 = cx0 >> 3, ty0 = cy0 >> 3, tw = (cx1 >> 3) - tx0 + 1, nt = tw * ((cy1 >> 3) - ty0 + 1);
        // the footprint's tiles, or the list of tiles with live rays when that is shorter
        const bool byList = nt > (int)liveCount;
        const int nIter = byList ? (int)liveCount : nt;
        for (int k0 = 0; k0 < nIter; k0 += 64) {
            const int k = k0 + lane;
            int tx = 0, ty = 0;
            bool pass = false;
            if (k < nIter) {
                if (byList) {
                    const uint32_t t = a.liveTiles[k];
                    tx = (int)(t % (uint32_t)a.tilesW);
                    ty = (int)(t / (uint32_t)a.tilesW);
                    pass = tx >= tx0 && tx < tx0 + tw && ty >= ty0 && ty <= (cy1 >> 3);
                } else {
                    tx = tx0 + k % tw;
                    ty = ty0 + k / tw;
                    pass = true;
                }
                pass = pass && raster_tile(a, tx, ty, czlo, czhi);
            }
            for (unsigned long long tm = __ballot(pass); tm; tm &= tm - 1ull) {
                const int src = __ffsll((long long)tm) - 1;
                const int x = __shfl(tx, src) * 8 + (lane & 7), y = __shfl(ty, src) * 8 + (lane >> 3);
                if (x >= cx0 && x <= cx1 && y >= cy0 && y <= cy1) tests += raster_texel<K>(a, x, y, w0, w1, w2, queue);
            }
        }
    }
    if (a.counters) {
        atomicAdd(&a.counters[3], (unsigned long long)tests);                        // exact tests
        if (i < a.nTris) atomicAdd(&a.counters[9], 1ull);                              // records read
    }
}

// The raster walk, then the resolve over its 64-bit keys
hipError_t launch_sd_walk_raster(const SDArgs& a, const SdPlan& pl, uint32_t N, const float4* queue, uint32_t* qctl,
                                 uint2* keys, hipStream_t s) {
    return sd_dispatch_kn(pl.K, N, [&](auto k, auto n) {
        constexpr int K = decltype(k)::value, N_ = decltype(n)::value, ROW = K <= 8 ? 8 : 16;
        hipLaunchKernelGGL((sd_raster_kernel<K>), dim3(pl.rasterBlocks), dim3(kRasterBlock), 0, s, a, queue, qctl);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((sd_resolve_row_kernel<K, N_, ROW, true>), dim3(pl.persistentBlocks), dim3(kBlock), 0, s, a,
                           queue, qctl, keys);
        return hipGetLastError();
    });
}

}  // namespace rsd
