// rsd_host.cpp -- librsd host entry points: errors, devices, scene upload (BVH build +
// HBM residency), camera and SVAO constant derivation.  No GPU work besides copies.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "bvh_refit.h"
#include "entry_grid.h"
#include "lbvh.h"
#include "rsd_internal.h"

namespace rsd {
namespace {
thread_local std::string g_last_error;
}
void set_error(const std::string& msg) { g_last_error = msg; }
rsd_status hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? RSD_ERR_OUT_OF_MEMORY : RSD_ERR_HIP;
}
}  // namespace rsd

using rsd::set_error;

extern "C" uint32_t rsd_abi_version(void) { return RSD_ABI_VERSION; }

extern "C" const char* rsd_last_error(void) { return rsd::g_last_error.c_str(); }

extern "C" rsd_status rsd_device_open(int hip_device, rsd_device** out) {
    if (!out) {
        set_error("rsd_device_open: out is null");
        return RSD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error("rsd_device_open: no HIP device available");
        return RSD_ERR_NO_DEVICE;
    }
    if (hip_device < 0 || hip_device >= n) {
        set_error("rsd_device_open: device index out of range");
        return RSD_ERR_INVALID_ARG;
    }
    RSD_HIP(hipSetDevice(hip_device));
    hipDeviceProp_t prop;
    RSD_HIP(hipGetDeviceProperties(&prop, hip_device));
    auto* d = new rsd_device;
    d->hip_device = hip_device;
    d->cu_count = prop.multiProcessorCount;
    *out = d;
    return RSD_OK;
}

extern "C" void rsd_device_close(rsd_device* dev) { delete dev; }

namespace {
// cgroup v2 CPU quota of this process ("max 100000" = none): ceil(quota / period) CPUs, or 0
unsigned cgroup_cpu_quota() {
    FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r");
    if (!f) return 0;
    char q[32] = {0};
    long long period = 0;
    const int n = std::fscanf(f, "%31s %lld", q, &period);
    std::fclose(f);
    if (n != 2 || period <= 0 || std::strcmp(q, "max") == 0) return 0;
    const long long quota = std::atoll(q);
    return quota > 0 ? (unsigned)((quota + period - 1) / period) : 0;
}

// Host threads of the BVH build: the CPUs this process may actually use -- its affinity mask (what a
// container or `taskset` grants) capped by the cgroup CPU quota (a GPU box shows 256 CPUs under a
// 16-CPU quota; bench.py's cpu_baseline counts cores the same way) -- or RSD_BUILD_THREADS.
unsigned build_threads() {
    if (const char* env = std::getenv("RSD_BUILD_THREADS"))
        if (int n = std::atoi(env); n > 0) return (unsigned)n;
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) n = (unsigned)CPU_COUNT(&set);
    if (const unsigned q = cgroup_cpu_quota()) n = std::min(n, q);
    return std::max(1u, n);
}
}  // namespace

namespace {
// the segment entry grid of `nodes` (the scene's wide nodes on the host) into a fresh device table, replacing
// the scene's (RSD_ENTRY_CELLS bounds its cells, 0 = none)
rsd_status upload_entry_grid(rsd_scene* s, const std::vector<float>& nodes, unsigned threads, const char* who) {
    uint64_t maxCells = 1ull << 21;
    if (const char* env = std::getenv("RSD_ENTRY_CELLS")) maxCells = (uint64_t)std::atoll(env);
    rsd::EntryGrid g;
    if (s->triangle_count && maxCells) g = rsd::build_entry_grid(nodes, s->tri_offset, maxCells, threads);
    void* d = nullptr;
    const size_t sb = g.slots.size() * 4, ib = g.items.size() * 4;
    if (g.cells) {
        hipError_t e = hipMalloc(&d, sb + ib);
        if (e == hipSuccess) e = hipMemcpy(d, g.slots.data(), sb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(static_cast<char*>(d) + sb, g.items.data(), ib, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return rsd::hip_fail(e, who);
        }
    }
    if (s->d_entry) {
        (void)hipFree(s->d_entry);
        s->device_bytes -= s->entry_bytes;
    }
    s->d_entry = d;
    s->entry_bytes = g.cells ? sb + ib : 0;
    s->entry_items_off = g.cells ? sb : 0;
    uint32_t bits = 0;
    while (g.cells && (4ull << bits) < g.slots.size()) ++bits;
    s->entry_bits = bits;
    s->entry_probe = g.cells ? g.max_probe : 0;
    s->entry_rmax = g.cells ? g.rmax : 0;
    s->entry_cells = g.cells;
    for (int k = 0; k < 3; ++k) s->entry_origin[k] = g.cells ? g.origin[k] : 0.0f;
    s->entry_extent = g.cells ? g.extent : 0.0f;
    s->entry_build_ms = g.cells ? g.build_ms : 0.0;
    s->device_bytes += s->entry_bytes;
    return RSD_OK;
}

// What a refit needs, in one allocation (rsd_internal.h DynamicData): the index buffer, the positions, and per
// wide node its parent, its count of inner children, a zeroed arrival counter and a tight box.
rsd_status upload_dynamic_data(rsd_scene* s, const rsd_scene_desc* desc, const rsd::FlatBvh& bvh) {
    const uint32_t nn = s->node_count, nt = desc->triangle_count, nv = desc->vertex_count;
    std::vector<uint32_t> parent(nn), inner(nn);
    if (!rsd::refit_topology(reinterpret_cast<const uint32_t*>(bvh.nodes.data()), nn, nt, parent.data(), inner.data())) {
        set_error("rsd_scene_upload_dynamic: the built tree is not one a refit can walk");
        return RSD_ERR_UNSUPPORTED;
    }
    const rsd::DynLayout lay = rsd::dyn_layout(nt, nv, nn);
    const size_t oInd = lay.indices, oPos = lay.positions, oPar = lay.parent, oInner = lay.inner, oArr = lay.arrive,
                 oTight = lay.tight, total = lay.total;
    char* d = nullptr;
    hipError_t e = hipMalloc(&d, total);
    if (e == hipSuccess) e = hipMemset(d, 0, total);
    if (e == hipSuccess && nt) e = hipMemcpy(d + oInd, desc->indices, 12 * (size_t)nt, hipMemcpyHostToDevice);
    if (e == hipSuccess && nv) e = hipMemcpy(d + oPos, desc->positions, 12 * (size_t)nv, hipMemcpyHostToDevice);
    if (e == hipSuccess && nn) e = hipMemcpy(d + oPar, parent.data(), 4 * (size_t)nn, hipMemcpyHostToDevice);
    if (e == hipSuccess && nn) e = hipMemcpy(d + oInner, inner.data(), 4 * (size_t)nn, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return rsd::hip_fail(e, "rsd_scene_upload_dynamic");
    }
    s->d_dyn = d;
    s->dyn.indices = reinterpret_cast<uint32_t*>(d + oInd);
    s->dyn.positions = reinterpret_cast<float*>(d + oPos);
    s->dyn.parent = reinterpret_cast<uint32_t*>(d + oPar);
    s->dyn.inner = reinterpret_cast<uint32_t*>(d + oInner);
    s->dyn.arrive = reinterpret_cast<uint32_t*>(d + oArr);
    s->dyn.tight = reinterpret_cast<uint32_t*>(d + oTight);
    s->dyn_bytes = total;
    s->device_bytes += total;
    return RSD_OK;
}

rsd_status scene_upload(rsd_device* dev, const rsd_scene_desc* desc, rsd_scene** out, bool dynamic);
}  // namespace

extern "C" rsd_status rsd_scene_upload(rsd_device* dev, const rsd_scene_desc* desc, rsd_scene** out) {
    return scene_upload(dev, desc, out, false);
}

namespace {
rsd_status scene_upload(rsd_device* dev, const rsd_scene_desc* desc, rsd_scene** out, bool dynamic) {
    if (!dev || !desc || !out || (desc->triangle_count && (!desc->positions || !desc->indices))) {
        set_error("rsd_scene_upload: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    for (uint64_t i = 0; i < 3ull * desc->triangle_count; ++i)
        if (desc->indices[i] >= desc->vertex_count) {
            set_error("rsd_scene_upload: index out of range of vertex_count");
            return RSD_ERR_INVALID_ARG;
        }
    if (desc->triangle_count >= (1u << 30)) {
        set_error("rsd_scene_upload: too many triangles");
        return RSD_ERR_UNSUPPORTED;
    }
    RSD_HIP(hipSetDevice(dev->hip_device));
    const unsigned threads = build_threads();
    rsd::BvhOptions opt;
    opt.split_budget = 0.0;  // a refit cannot reproduce the clipped boxes of spatial-split references
    rsd::FlatBvh bvh = rsd::build_bvh(desc->positions, desc->vertex_count, desc->indices, desc->triangle_count,
                                      desc->triangle_flags, threads, opt);
    if (dynamic && (bvh.stats.spatial_splits != 0 || bvh.stats.references != desc->triangle_count)) {
        set_error("rsd_scene_upload_dynamic: the tree has spatial splits, which a refit cannot keep");
        return RSD_ERR_UNSUPPORTED;
    }
    auto* s = new rsd_scene;
    s->dev = dev;
    s->triangle_count = desc->triangle_count;
    s->vertex_count = desc->vertex_count;
    s->node_count = (uint32_t)(bvh.nodes.size() / 32);
    s->stats = bvh.stats;
    s->build_threads = threads;
    // one allocation: wide nodes, then triangle records, then 12 x 16 B of padding so a
    // traversal step may always fetch 192 B (DESIGN.md "BVH layout in HBM")
    const size_t nb = bvh.nodes.size() * sizeof(float), tb = bvh.tris.size() * sizeof(float);
    const size_t total = nb + tb + 12 * 16;
    s->tri_offset = (uint32_t)(bvh.nodes.size() / 4);
    hipError_t e = hipMalloc(&s->d_nodes, total);
    if (e == hipSuccess) e = hipMemset(s->d_nodes, 0, total);
    if (e == hipSuccess) e = hipMemcpy(s->d_nodes, bvh.nodes.data(), nb, hipMemcpyHostToDevice);
    if (e == hipSuccess && tb)
        e = hipMemcpy(reinterpret_cast<char*>(s->d_nodes) + nb, bvh.tris.data(), tb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        rsd_status st = rsd::hip_fail(e, "rsd_scene_upload");
        (void)hipFree(s->d_nodes);
        delete s;
        return st;
    }
    s->d_tris = s->d_nodes + s->tri_offset;
    s->device_bytes = total;
    s->bvh_bytes = total;
    if (desc->triangle_count) {
        // primitive id -> triangle record (record r holds prim in v0.w): the raster SD walk keys its
        // hits by (t, prim) and its resolve pass needs the record of each key
        std::vector<uint32_t> pr(desc->triangle_count, 0u);
        for (uint32_t r = 0; r < desc->triangle_count; ++r) {
            uint32_t prim;
            std::memcpy(&prim, &bvh.tris[(size_t)r * 12 + 3], 4);
            pr[prim] = r;
        }
        e = hipMalloc(&s->d_prim_rec, pr.size() * 4);
        if (e == hipSuccess) e = hipMemcpy(s->d_prim_rec, pr.data(), pr.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rsd_status st = rsd::hip_fail(e, "rsd_scene_upload (prim map)");
            (void)hipFree(s->d_prim_rec);
            (void)hipFree(s->d_nodes);
            delete s;
            return st;
        }
        s->device_bytes += pr.size() * 4;
    }
    // segment entry grid
    rsd_status st = upload_entry_grid(s, bvh.nodes, threads, "rsd_scene_upload (entry grid)");
    if (st == RSD_OK && dynamic) st = upload_dynamic_data(s, desc, bvh);
    if (st != RSD_OK) {
        rsd_scene_release(s);
        return st;
    }
    *out = s;
    return RSD_OK;
}
}  // namespace

namespace {
// MaterialHeader stores the alpha threshold as float16 (MaterialData.slang:99): round to
// nearest even at half precision, then widen.  A NaN threshold stays a NaN: `alpha < threshold` is then false and the
// hit is kept (rsd.h rsd_material).
float round_half(float f) {
    if (f != f) return f;
    const float a = std::fabs(f);
    if (a >= 65520.0f) return std::copysign(INFINITY, f);
    int e = 0;
    (void)std::frexp(a, &e);                  // a = m 2^e, m in [0.5, 1)
    const int q = std::max(e - 11, -24);      // quantum exponent: 10 fraction bits, subnormals
    return std::ldexp(std::nearbyint(std::ldexp(f, -q)), q);
}

// The 2x2 box mip chain of one R8 texture (DESIGN.md "Alpha test"): level l+1 texel (x, y)
// averages level l texels (2x..2x+1, 2y..2y+1), clamped to the level, (a+b+c+d+2)/4.
void build_mips(const rsd_alpha_texture& t, std::vector<uint8_t>& out, uint32_t& mips) {
    uint32_t w = t.width, h = t.height;
    size_t base = out.size();
    out.insert(out.end(), t.alpha, t.alpha + (size_t)w * h);
    mips = 1;
    while (w > 1 || h > 1) {
        const uint32_t nw = std::max(1u, w >> 1), nh = std::max(1u, h >> 1);
        const size_t nbase = out.size();
        out.resize(nbase + (size_t)nw * nh);
        for (uint32_t y = 0; y < nh; ++y)
            for (uint32_t x = 0; x < nw; ++x) {
                const uint32_t x0 = std::min(2 * x, w - 1), x1 = std::min(2 * x + 1, w - 1);
                const uint32_t y0 = std::min(2 * y, h - 1), y1 = std::min(2 * y + 1, h - 1);
                const uint8_t* l = out.data() + base;
                const uint32_t sum = l[(size_t)y0 * w + x0] + l[(size_t)y0 * w + x1] + l[(size_t)y1 * w + x0] +
                                     l[(size_t)y1 * w + x1] + 2;
                out[nbase + (size_t)y * nw + x] = (uint8_t)(sum / 4);
            }
        base = nbase;
        w = nw;
        h = nh;
        ++mips;
    }
}
}  // namespace

namespace {
rsd_status scene_upload_alpha(rsd_device* dev, const rsd_scene_desc* desc, const rsd_alpha_desc* alpha, rsd_scene** out,
                              bool dynamic) {
    if (!alpha) return scene_upload(dev, desc, out, dynamic);
    if (!dev || !desc || !out || !alpha->triangle_material || !alpha->materials || alpha->material_count == 0 ||
        (desc->vertex_count && !alpha->texcoords) || (alpha->texture_count && !alpha->textures)) {
        set_error("rsd_scene_upload_alpha: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; i < alpha->texture_count; ++i) {
        const rsd_alpha_texture& t = alpha->textures[i];
        if (t.width == 0 || t.height == 0 || !t.alpha || t.width > 32768 || t.height > 32768) {
            set_error("rsd_scene_upload_alpha: texture " + std::to_string(i) + " is empty or too large");
            return RSD_ERR_INVALID_ARG;
        }
    }
    for (uint32_t i = 0; i < alpha->material_count; ++i) {
        const uint32_t tex = alpha->materials[i].texture;
        if (tex != RSD_NO_TEXTURE && tex >= alpha->texture_count) {
            set_error("rsd_scene_upload_alpha: material " + std::to_string(i) + " names a missing texture");
            return RSD_ERR_INVALID_ARG;
        }
    }
    for (uint32_t i = 0; i < desc->triangle_count; ++i)
        if (alpha->triangle_material[i] >= alpha->material_count) {
            set_error("rsd_scene_upload_alpha: triangle_material out of range of material_count");
            return RSD_ERR_INVALID_ARG;
        }
    // the texcoord contract (rsd.h rsd_alpha_desc.texcoords): tex_split (tex_sample.h) converts floor(u W - 0.5) to an
    // int, W <= 32768, so a sampled coordinate is finite and within +-32768 -- |u W| + 2 <= 2^30 + 2, a factor of two
    // below INT_MAX for the interpolation's rounding.  Only the vertices of textured alpha-masked triangles are sampled.
    // (An index past vertex_count is scene_upload's to refuse.)
    if (desc->triangle_flags && desc->indices && alpha->texcoords)
        for (uint32_t t = 0; t < desc->triangle_count; ++t) {
            if (!(desc->triangle_flags[t] & RSD_TRI_ALPHA_MASK) ||
                alpha->materials[alpha->triangle_material[t]].texture == RSD_NO_TEXTURE)
                continue;
            for (int j = 0; j < 3; ++j) {
                const uint32_t v = desc->indices[3 * (size_t)t + j];
                if (v >= desc->vertex_count) continue;
                const float tu = alpha->texcoords[2 * (size_t)v], tv = alpha->texcoords[2 * (size_t)v + 1];
                if (!(std::fabs(tu) <= 32768.0f) || !(std::fabs(tv) <= 32768.0f)) {  // false for a NaN
                    set_error("rsd_scene_upload_alpha: vertex " + std::to_string(v) + " (triangle " + std::to_string(t) +
                              ") has a texcoord that is not finite or outside [-32768, 32768]");
                    return RSD_ERR_INVALID_ARG;
                }
            }
        }
    rsd_status st = scene_upload(dev, desc, out, dynamic);
    if (st != RSD_OK) return st;
    rsd_scene* s = *out;
    const uint32_t nt = desc->triangle_count, nm = alpha->material_count, nx = alpha->texture_count;
    // per-primitive texture coordinates (Scene::computeVertexData reads them per vertex)
    std::vector<float> uv(6 * (size_t)nt);
    for (size_t t = 0; t < nt; ++t)
        for (int j = 0; j < 3; ++j) {
            const uint32_t v = desc->indices[3 * t + j];
            uv[6 * t + 2 * j] = alpha->texcoords[2 * (size_t)v];
            uv[6 * t + 2 * j + 1] = alpha->texcoords[2 * (size_t)v + 1];
        }
    std::vector<float> mats(4 * (size_t)nm);
    for (uint32_t i = 0; i < nm; ++i) {
        const rsd_material& m = alpha->materials[i];
        mats[4 * i] = round_half(m.alpha_threshold);
        mats[4 * i + 1] = m.alpha;
        std::memcpy(&mats[4 * i + 2], &m.texture, 4);
        mats[4 * i + 3] = 0.0f;
    }
    std::vector<uint32_t> texs(4 * (size_t)nx);
    std::vector<uint8_t> texels;
    for (uint32_t i = 0; i < nx; ++i) {
        texs[4 * i] = alpha->textures[i].width;
        texs[4 * i + 1] = alpha->textures[i].height;
        texs[4 * i + 3] = (uint32_t)texels.size();
        build_mips(alpha->textures[i], texels, texs[4 * i + 2]);
        if (texels.size() >= (1ull << 32)) {
            rsd_scene_release(s);
            *out = nullptr;
            set_error("rsd_scene_upload_alpha: more than 4 GiB of texels");
            return RSD_ERR_UNSUPPORTED;
        }
    }
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t oUV = 0, oMat = al(uv.size() * 4), oMats = oMat + al(4 * (size_t)nt), oTex = oMats + al(mats.size() * 4),
                 oTexel = oTex + al(texs.size() * 4), total = oTexel + al(texels.size() + 16);
    char* d = nullptr;
    hipError_t e = hipMalloc(&d, total);
    if (e == hipSuccess) e = hipMemset(d, 0, total);
    if (e == hipSuccess && nt) e = hipMemcpy(d + oUV, uv.data(), uv.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nt) e = hipMemcpy(d + oMat, alpha->triangle_material, 4 * (size_t)nt, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + oMats, mats.data(), mats.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nx) e = hipMemcpy(d + oTex, texs.data(), texs.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !texels.empty()) e = hipMemcpy(d + oTexel, texels.data(), texels.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        st = rsd::hip_fail(e, "rsd_scene_upload_alpha");
        (void)hipFree(d);
        rsd_scene_release(s);
        *out = nullptr;
        return st;
    }
    s->d_alpha = d;
    s->alpha.triUV = reinterpret_cast<const float*>(d + oUV);
    s->alpha.triMat = reinterpret_cast<const uint32_t*>(d + oMat);
    s->alpha.materials = reinterpret_cast<const float4*>(d + oMats);
    s->alpha.textures = reinterpret_cast<const uint4*>(d + oTex);
    s->alpha.texels = reinterpret_cast<const uint8_t*>(d + oTexel);
    s->device_bytes += total;
    return RSD_OK;
}
}  // namespace

extern "C" rsd_status rsd_scene_upload_alpha(rsd_device* dev, const rsd_scene_desc* desc, const rsd_alpha_desc* alpha,
                                             rsd_scene** out) {
    return scene_upload_alpha(dev, desc, alpha, out, false);
}

extern "C" rsd_status rsd_scene_upload_dynamic(rsd_device* dev, const rsd_scene_desc* desc, const rsd_alpha_desc* alpha,
                                               rsd_scene** out) {
    return scene_upload_alpha(dev, desc, alpha, out, true);
}

extern "C" float rsd_ray_cone_spread(float focal_length, uint32_t height) {
    // every SD trace asks for it with the frame's (focal length, height): keep the last answer per thread
    // (the decimal round trip below costs about as much as a kernel launch on the host)
    thread_local float lastF = -1.0f, lastS = 0.0f;
    thread_local uint32_t lastH = 0;
    if (focal_length == lastF && height == lastH) return lastS;
    const float fovY = 2.0f * std::atan(0.5f * 24.0f / focal_length);  // focalLengthToFovY(f, kDefaultFrameHeight)
    const float angle = std::atan(2.0f * std::tan(fovY * 0.5f) / (float)height);
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%f", (double)angle);  // std::to_string(float)
    lastS = std::strtof(buf, nullptr);
    lastF = focal_length;
    lastH = height;
    return lastS;
}

extern "C" rsd_status rsd_scene_info_get(const rsd_scene* s, rsd_scene_info* out) {
    if (!s || !out) {
        set_error("rsd_scene_info_get: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    out->triangle_count = s->triangle_count;
    out->node_count = s->node_count;
    out->max_depth = s->stats.max_depth;
    out->wide_depth = s->stats.wide_depth;
    out->leaf_count = s->stats.leaves;
    out->sah_cost = s->stats.sah_cost;
    out->build_ms = s->stats.build_ms + s->entry_build_ms;
    out->device_bytes = s->device_bytes;
    out->build_threads = s->build_threads;
    out->entry_cells = s->entry_cells;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_dynamic_info_get(const rsd_scene* s, rsd_scene_dynamic_info* out) {
    if (!s || !out) {
        set_error("rsd_scene_dynamic_info_get: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    out->dynamic = s->d_dyn ? 1u : 0u;
    out->entry_grid_current = s->entry_stale ? 0u : 1u;
    out->updates = s->updates;
    out->dynamic_bytes = s->dyn_bytes;
    return RSD_OK;
}

namespace {
rsd_status require_dynamic(const rsd_scene* s, const char* who) {
    if (!s) {
        set_error(std::string(who) + ": null scene");
        return RSD_ERR_INVALID_ARG;
    }
    if (!s->d_dyn) {
        set_error(std::string(who) + ": the scene is not dynamic (upload it with rsd_scene_upload_dynamic)");
        return RSD_ERR_INVALID_ARG;
    }
    return RSD_OK;
}

// free the morph table of a scene (the caller has waited for the device)
void drop_morph(rsd_scene* s) {
    if (!s->d_morph) return;
    (void)hipFree(s->d_morph);
    s->device_bytes -= s->morph_bytes;
    s->d_morph = nullptr;
    s->morph = rsd::MorphData{};
    s->morph_bytes = 0;
}
}  // namespace

extern "C" rsd_status rsd_scene_update_positions(rsd_scene* s, const float* positions, uint32_t vertex_count,
                                                 uint32_t positions_on_device, rsd_stream stream) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_update_positions"); st != RSD_OK) return st;
    if (vertex_count != s->vertex_count) {
        set_error("rsd_scene_update_positions: vertex_count " + std::to_string(vertex_count) + " is not the upload's " +
                  std::to_string(s->vertex_count));
        return RSD_ERR_INVALID_ARG;
    }
    if (!positions && vertex_count) {
        set_error("rsd_scene_update_positions: null positions");
        return RSD_ERR_INVALID_ARG;
    }
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    hipStream_t hs = (hipStream_t)stream;
    if (vertex_count)
        RSD_HIP(hipMemcpyAsync(s->dyn.positions, positions, 12 * (size_t)vertex_count,
                               positions_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, hs));
    s->entry_stale = s->entry_stale || s->d_entry != nullptr;
    ++s->updates;
    return rsd::refit_enqueue(s, hs);
}

extern "C" rsd_status rsd_scene_update_subset(rsd_scene* s, const uint32_t* d_vertex_ids, const float* d_positions,
                                              uint32_t count, rsd_stream stream) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_update_subset"); st != RSD_OK) return st;
    if (count && (!d_vertex_ids || !d_positions)) {
        set_error("rsd_scene_update_subset: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    hipStream_t hs = (hipStream_t)stream;
    if (rsd_status st = rsd::refit_scatter_enqueue(s, d_vertex_ids, d_positions, count, hs); st != RSD_OK) return st;
    s->entry_stale = s->entry_stale || s->d_entry != nullptr;
    ++s->updates;
    return rsd::refit_enqueue(s, hs);
}

extern "C" rsd_status rsd_scene_attach_rig(rsd_scene* s, const rsd_rig_desc* rig) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_attach_rig"); st != RSD_OK) return st;
    auto refuse = [](const std::string& why) {
        set_error("rsd_scene_attach_rig: " + why);
        return RSD_ERR_INVALID_ARG;
    };
    if (!rig) return refuse("null rig");
    const uint32_t n = rig->count, nm = rig->matrix_count, nv = s->vertex_count;
    if (n && (!rig->vertex_ids || !rig->matrix_ids || !rig->weights)) return refuse("null argument");
    if (n && !nm) return refuse("matrix_count is 0 with animated vertices");
    {
        std::vector<uint8_t> seen(nv, 0);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t v = rig->vertex_ids[i];
            if (v >= nv)
                return refuse("vertex id " + std::to_string(v) + " is out of range of vertex_count " + std::to_string(nv));
            if (seen[v]) return refuse("vertex " + std::to_string(v) + " is named twice");
            seen[v] = 1;
            for (int k = 0; k < 4; ++k)
                if (rig->matrix_ids[4 * (size_t)i + k] >= nm)
                    return refuse("matrix id " + std::to_string(rig->matrix_ids[4 * (size_t)i + k]) +
                                  " is out of range of matrix_count " + std::to_string(nm));
        }
    }
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    // synchronous: updates enqueued so far have run before the rest positions are read and before the rig
    // a pose in flight reads is freed
    RSD_HIP(hipDeviceSynchronize());
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t oVid = 0, oMid = al(4 * (size_t)n), oW = oMid + al(16 * (size_t)n), oRest = oW + al(16 * (size_t)n),
                 oMat = oRest + al(12 * (size_t)n), total = oMat + al(48 * (size_t)nm);
    std::vector<float> rest(3 * (size_t)n);
    if (n && rig->rest_positions) {
        std::memcpy(rest.data(), rig->rest_positions, 12 * (size_t)n);
    } else if (n) {
        std::vector<float> all(3 * (size_t)nv);
        RSD_HIP(hipMemcpy(all.data(), s->dyn.positions, 12 * (size_t)nv, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) rest[3 * (size_t)i + k] = all[3 * (size_t)rig->vertex_ids[i] + k];
    }
    char* d = nullptr;
    hipError_t e = hipMalloc(&d, total ? total : 256);
    if (e == hipSuccess && total) e = hipMemset(d, 0, total);
    if (e == hipSuccess && n) e = hipMemcpy(d + oVid, rig->vertex_ids, 4 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(d + oMid, rig->matrix_ids, 16 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(d + oW, rig->weights, 16 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(d + oRest, rest.data(), 12 * (size_t)n, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return rsd::hip_fail(e, "rsd_scene_attach_rig");
    }
    if (s->d_rig) {
        (void)hipFree(s->d_rig);
        s->device_bytes -= s->rig_bytes;
    }
    drop_morph(s);  // the table was indexed by the old rig's vertices
    s->d_rig = d;
    s->rig.count = n;
    s->rig.matrix_count = nm;
    s->rig.vertex_ids = reinterpret_cast<uint32_t*>(d + oVid);
    s->rig.matrix_ids = reinterpret_cast<uint32_t*>(d + oMid);
    s->rig.weights = reinterpret_cast<float*>(d + oW);
    s->rig.rest = reinterpret_cast<float*>(d + oRest);
    s->rig.matrices = reinterpret_cast<float*>(d + oMat);
    s->rig_bytes = total ? total : 256;
    s->device_bytes += s->rig_bytes;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_update_pose(rsd_scene* s, const float* matrices, uint32_t matrix_count,
                                            uint32_t matrices_on_device, rsd_stream stream) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_update_pose"); st != RSD_OK) return st;
    if (!s->d_rig) {
        set_error("rsd_scene_update_pose: the scene has no rig (rsd_scene_attach_rig)");
        return RSD_ERR_INVALID_ARG;
    }
    if (matrix_count != s->rig.matrix_count) {
        set_error("rsd_scene_update_pose: matrix_count " + std::to_string(matrix_count) + " is not the rig's " +
                  std::to_string(s->rig.matrix_count));
        return RSD_ERR_INVALID_ARG;
    }
    if (!matrices && matrix_count) {
        set_error("rsd_scene_update_pose: null matrices");
        return RSD_ERR_INVALID_ARG;
    }
    if (matrices_on_device && reinterpret_cast<uintptr_t>(matrices) % 16 != 0) {
        set_error("rsd_scene_update_pose: device matrices must be 16-byte aligned");
        return RSD_ERR_INVALID_ARG;
    }
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    hipStream_t hs = (hipStream_t)stream;
    const float* d_matrices = matrices;
    if (!matrices_on_device) {
        if (matrix_count)
            RSD_HIP(hipMemcpyAsync(s->rig.matrices, matrices, 48 * (size_t)matrix_count, hipMemcpyHostToDevice, hs));
        d_matrices = s->rig.matrices;
    }
    if (rsd_status st = rsd::pose_enqueue(s, d_matrices, hs); st != RSD_OK) return st;
    s->entry_stale = s->entry_stale || s->d_entry != nullptr;
    ++s->updates;
    return rsd::refit_enqueue(s, hs);
}

extern "C" rsd_status rsd_scene_rig_info_get(const rsd_scene* s, rsd_scene_rig_info* out) {
    if (!s || !out) {
        set_error("rsd_scene_rig_info_get: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    out->attached = s->d_rig ? 1u : 0u;
    out->count = s->rig.count;
    out->matrix_count = s->rig.matrix_count;
    out->reserved = 0;
    out->rig_bytes = s->rig_bytes;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_attach_morph(rsd_scene* s, const rsd_morph_desc* m) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_attach_morph"); st != RSD_OK) return st;
    auto refuse = [](const std::string& why) {
        set_error("rsd_scene_attach_morph: " + why);
        return RSD_ERR_INVALID_ARG;
    };
    if (!s->d_rig) return refuse("the scene has no rig (rsd_scene_attach_rig)");
    if (!m) return refuse("null morph table");
    const uint32_t n = m->count, nw = m->weight_count;
    if (n != s->rig.count)
        return refuse("count " + std::to_string(n) + " is not the rig's " + std::to_string(s->rig.count));
    if (!m->offsets) return refuse("null offsets");
    if (m->offsets[0] != 0) return refuse("offsets[0] is " + std::to_string(m->offsets[0]) + ", not 0");
    for (uint32_t i = 0; i < n; ++i)
        if (m->offsets[i + 1] < m->offsets[i])
            return refuse("offsets decrease at rig vertex " + std::to_string(i) + " (" + std::to_string(m->offsets[i]) +
                          " -> " + std::to_string(m->offsets[i + 1]) + ")");
    const uint32_t ne = m->offsets[n];
    if (ne && (!m->weight_ids || !m->deltas)) return refuse("null argument");
    for (uint32_t e = 0; e < ne; ++e)
        if (m->weight_ids[e] >= nw)
            return refuse("weight id " + std::to_string(m->weight_ids[e]) + " is out of range of weight_count " +
                          std::to_string(nw));
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    // synchronous: a pose in flight has read the table it is about to lose
    RSD_HIP(hipDeviceSynchronize());
    if (!ne) {
        drop_morph(s);
        return RSD_OK;
    }
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t oOff = 0, oEnt = al(4 * ((size_t)n + 1)), oW = oEnt + al(16 * (size_t)ne), total = oW + al(4 * (size_t)nw);
    std::vector<uint32_t> ent(4 * (size_t)ne);
    for (uint32_t e = 0; e < ne; ++e) {
        ent[4 * (size_t)e] = m->weight_ids[e];
        std::memcpy(&ent[4 * (size_t)e + 1], m->deltas + 3 * (size_t)e, 12);
    }
    char* d = nullptr;
    hipError_t e = hipMalloc(&d, total);
    if (e == hipSuccess) e = hipMemset(d, 0, total);
    if (e == hipSuccess) e = hipMemcpy(d + oOff, m->offsets, 4 * ((size_t)n + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + oEnt, ent.data(), 16 * (size_t)ne, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return rsd::hip_fail(e, "rsd_scene_attach_morph");
    }
    drop_morph(s);
    s->d_morph = d;
    s->morph.count = n;
    s->morph.weight_count = nw;
    s->morph.entry_count = ne;
    s->morph.offsets = reinterpret_cast<uint32_t*>(d + oOff);
    s->morph.entries = reinterpret_cast<uint4*>(d + oEnt);
    s->morph.weights = reinterpret_cast<float*>(d + oW);
    s->morph_bytes = total;
    s->device_bytes += total;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_update_pose_morph(rsd_scene* s, const float* matrices, uint32_t matrix_count,
                                                  const float* weights, uint32_t weight_count, uint32_t on_device,
                                                  rsd_stream stream) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_update_pose_morph"); st != RSD_OK) return st;
    if (!s->d_morph) {
        set_error("rsd_scene_update_pose_morph: the scene has no morph table (rsd_scene_attach_morph)");
        return RSD_ERR_INVALID_ARG;
    }
    if (weight_count != s->morph.weight_count) {
        set_error("rsd_scene_update_pose_morph: weight_count " + std::to_string(weight_count) + " is not the table's " +
                  std::to_string(s->morph.weight_count));
        return RSD_ERR_INVALID_ARG;
    }
    if (matrix_count != s->rig.matrix_count) {
        set_error("rsd_scene_update_pose_morph: matrix_count " + std::to_string(matrix_count) + " is not the rig's " +
                  std::to_string(s->rig.matrix_count));
        return RSD_ERR_INVALID_ARG;
    }
    if ((!matrices && matrix_count) || (!weights && weight_count)) {
        set_error("rsd_scene_update_pose_morph: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    if (on_device && reinterpret_cast<uintptr_t>(matrices) % 16 != 0) {
        set_error("rsd_scene_update_pose_morph: device matrices must be 16-byte aligned");
        return RSD_ERR_INVALID_ARG;
    }
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    hipStream_t hs = (hipStream_t)stream;
    // the weights always land in the scene's table: rsd_scene_update_pose reads them there later
    if (weight_count)
        RSD_HIP(hipMemcpyAsync(s->morph.weights, weights, 4 * (size_t)weight_count,
                               on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, hs));
    const float* d_matrices = matrices;
    if (!on_device) {
        if (matrix_count)
            RSD_HIP(hipMemcpyAsync(s->rig.matrices, matrices, 48 * (size_t)matrix_count, hipMemcpyHostToDevice, hs));
        d_matrices = s->rig.matrices;
    }
    if (rsd_status st = rsd::pose_enqueue(s, d_matrices, hs); st != RSD_OK) return st;
    s->entry_stale = s->entry_stale || s->d_entry != nullptr;
    ++s->updates;
    return rsd::refit_enqueue(s, hs);
}

extern "C" rsd_status rsd_scene_morph_info_get(const rsd_scene* s, rsd_scene_morph_info* out) {
    if (!s || !out) {
        set_error("rsd_scene_morph_info_get: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    out->attached = s->d_morph ? 1u : 0u;
    out->count = s->morph.count;
    out->weight_count = s->morph.weight_count;
    out->entry_count = s->morph.entry_count;
    out->morph_bytes = s->morph_bytes;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_track_motion(rsd_scene* s) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_track_motion"); st != RSD_OK) return st;
    if (s->dyn.prev_positions) return RSD_OK;
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    // synchronous: updates enqueued so far have run before the positions are copied
    RSD_HIP(hipDeviceSynchronize());
    const size_t bytes = 12 * (size_t)s->vertex_count;
    float* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes ? bytes : 256);
    if (e == hipSuccess && bytes) e = hipMemcpy(d, s->dyn.positions, bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(d);
        return rsd::hip_fail(e, "rsd_scene_track_motion");
    }
    s->dyn.prev_positions = d;
    s->motion_bytes = bytes ? bytes : 256;
    s->device_bytes += s->motion_bytes;
    s->motion_seen_updates = s->updates;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_motion_begin_frame(rsd_scene* s, rsd_stream stream) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_motion_begin_frame"); st != RSD_OK) return st;
    if (!s->dyn.prev_positions) {
        set_error("rsd_scene_motion_begin_frame: motion is not tracked (rsd_scene_track_motion)");
        return RSD_ERR_INVALID_ARG;
    }
    if (s->motion_seen_updates == s->updates) return RSD_OK;  // no update since the last snapshot: already equal
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    if (rsd_status st = rsd::motion_snapshot_enqueue(s, (hipStream_t)stream); st != RSD_OK) return st;
    s->motion_seen_updates = s->updates;
    ++s->motion_snapshots;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_motion_info_get(const rsd_scene* s, rsd_scene_motion_info* out) {
    if (!s || !out) {
        set_error("rsd_scene_motion_info_get: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    out->tracked = s->dyn.prev_positions ? 1u : 0u;
    out->reserved = 0;
    out->snapshots = s->motion_snapshots;
    out->motion_bytes = s->motion_bytes;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_rebuild_entry_grid(rsd_scene* s) {
    if (!s) {
        set_error("rsd_scene_rebuild_entry_grid: null scene");
        return RSD_ERR_INVALID_ARG;
    }
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    // synchronous: every update and every trace enqueued so far has finished before the nodes are read
    // back and before the table those traces read is freed
    RSD_HIP(hipDeviceSynchronize());
    std::vector<float> nodes(4 * (size_t)s->tri_offset);
    if (!nodes.empty()) RSD_HIP(hipMemcpy(nodes.data(), s->d_nodes, nodes.size() * 4, hipMemcpyDeviceToHost));
    rsd_status st = upload_entry_grid(s, nodes, s->build_threads ? s->build_threads : build_threads(),
                                      "rsd_scene_rebuild_entry_grid");
    if (st != RSD_OK) return st;
    s->entry_stale = false;
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_rebuild_bvh(rsd_scene* s) {
    if (rsd_status st = require_dynamic(s, "rsd_scene_rebuild_bvh"); st != RSD_OK) return st;
    if (s->triangle_count > rsd::kLbvhMaxTriangles ||
        rsd::lbvh_depth_bound(s->triangle_count) > rsd::kLbvhMaxWideDepth) {
        set_error("rsd_scene_rebuild_bvh: too many triangles for the walks' stacks");
        return RSD_ERR_UNSUPPORTED;
    }
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    return rsd::lbvh_rebuild(s);
}

extern "C" rsd_status rsd_scene_rebuild_info_get(const rsd_scene* s, rsd_scene_rebuild_info* out) {
    if (!s || !out) {
        set_error("rsd_scene_rebuild_info_get: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    out->rebuilds = s->rebuilds;
    out->node_count = s->node_count;
    out->wide_depth = s->stats.wide_depth;
    out->device_ms = s->rebuild_ms;
    return RSD_OK;
}

extern "C" rsd_status rsd_bvh_build_lbvh(const rsd_scene_desc* desc, void* dst, uint64_t capacity, uint64_t* bytes,
                                         uint32_t* tri_offset) {
    if (!desc || !bytes || (desc->triangle_count && (!desc->positions || !desc->indices))) {
        set_error("rsd_bvh_build_lbvh: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    if (desc->triangle_count > rsd::kLbvhMaxTriangles ||
        rsd::lbvh_depth_bound(desc->triangle_count) > rsd::kLbvhMaxWideDepth) {
        set_error("rsd_bvh_build_lbvh: too many triangles for the walks' stacks");
        return RSD_ERR_UNSUPPORTED;
    }
    for (uint64_t i = 0; i < 3ull * desc->triangle_count; ++i)
        if (desc->indices[i] >= desc->vertex_count) {
            set_error("rsd_bvh_build_lbvh: index out of range of vertex_count");
            return RSD_ERR_INVALID_ARG;
        }
    std::vector<uint32_t> words;
    const rsd::LbvhResult res = rsd::lbvh_build_host(desc->positions, desc->vertex_count, desc->indices,
                                                     desc->triangle_count, desc->triangle_flags, words);
    *bytes = words.size() * 4;  // the layout of rsd_scene_upload's allocation
    if (tri_offset) *tri_offset = 8 * res.node_count;
    if (!dst) return RSD_OK;
    if (capacity < *bytes) {
        set_error("rsd_bvh_build_lbvh: capacity below the BVH size");
        return RSD_ERR_INVALID_ARG;
    }
    std::memcpy(dst, words.data(), *bytes);
    return RSD_OK;
}

extern "C" rsd_status rsd_bvh_refit(const void* bvh, uint64_t bvh_bytes, uint32_t tri_offset, const uint32_t* indices,
                                    uint32_t triangle_count, const float* positions, uint32_t vertex_count, void* dst) {
    const uint32_t nt = triangle_count;
    if (!bvh || !dst || (nt && (!indices || !positions))) {
        set_error("rsd_bvh_refit: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    const uint64_t nodeBytes = 16ull * tri_offset;
    if (tri_offset % 8 != 0 || bvh_bytes < nodeBytes + 12 * 16 || (bvh_bytes - nodeBytes - 12 * 16) % 48 != 0) {
        set_error("rsd_bvh_refit: bvh_bytes / tri_offset are not those of rsd_bvh_build");
        return RSD_ERR_INVALID_ARG;
    }
    const uint64_t records = (bvh_bytes - nodeBytes - 12 * 16) / 48;
    const uint32_t nn = tri_offset / 8;
    const uint32_t* src = static_cast<const uint32_t*>(bvh);
    // a triangle with several records (spatial splits) carries clipped boxes a refit cannot reproduce
    std::vector<uint8_t> seen(nt, 0);
    bool split = records != nt;
    for (uint64_t r = 0; r < records && !split; ++r) {
        const uint32_t prim = src[4 * (size_t)tri_offset + 12 * r + 3];
        if (prim >= nt) {
            set_error("rsd_bvh_refit: a record's primitive id is out of range of triangle_count");
            return RSD_ERR_INVALID_ARG;
        }
        split = seen[prim] != 0;
        seen[prim] = 1;
    }
    if (split) {
        set_error("rsd_bvh_refit: the tree has spatial splits (several records of one triangle)");
        return RSD_ERR_UNSUPPORTED;
    }
    for (uint64_t i = 0; i < 3ull * nt; ++i)
        if (indices[i] >= vertex_count) {
            set_error("rsd_bvh_refit: index out of range of vertex_count");
            return RSD_ERR_INVALID_ARG;
        }
    std::vector<uint32_t> parent(nn), inner(nn);
    if (!rsd::refit_topology(src, nn, nt, parent.data(), inner.data())) {
        set_error("rsd_bvh_refit: not a tree of rsd_bvh_build");
        return RSD_ERR_INVALID_ARG;
    }
    if (dst != bvh) std::memmove(dst, bvh, bvh_bytes);
    rsd::refit_host(static_cast<uint32_t*>(dst), nn, indices, nt, positions);
    return RSD_OK;
}

extern "C" rsd_status rsd_bvh_build(const rsd_scene_desc* desc, void* dst, uint64_t capacity, uint64_t* bytes,
                                    uint32_t* tri_offset) {
    if (!desc || !bytes || (desc->triangle_count && (!desc->positions || !desc->indices))) {
        set_error("rsd_bvh_build: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    for (uint64_t i = 0; i < 3ull * desc->triangle_count; ++i)
        if (desc->indices[i] >= desc->vertex_count) {
            set_error("rsd_bvh_build: index out of range of vertex_count");
            return RSD_ERR_INVALID_ARG;
        }
    rsd::FlatBvh bvh = rsd::build_bvh(desc->positions, desc->vertex_count, desc->indices, desc->triangle_count,
                                      desc->triangle_flags, build_threads());
    const size_t nb = bvh.nodes.size() * sizeof(float), tb = bvh.tris.size() * sizeof(float);
    *bytes = nb + tb + 12 * 16;  // the layout of rsd_scene_upload's allocation
    if (tri_offset) *tri_offset = (uint32_t)(bvh.nodes.size() / 4);
    if (!dst) return RSD_OK;
    if (capacity < *bytes) {
        set_error("rsd_bvh_build: capacity below the BVH size");
        return RSD_ERR_INVALID_ARG;
    }
    std::memcpy(dst, bvh.nodes.data(), nb);
    if (tb) std::memcpy(static_cast<char*>(dst) + nb, bvh.tris.data(), tb);
    std::memset(static_cast<char*>(dst) + nb + tb, 0, 12 * 16);
    return RSD_OK;
}

extern "C" rsd_status rsd_scene_export_bvh(const rsd_scene* s, void* dst, uint64_t capacity, uint64_t* bytes,
                                           uint32_t* tri_offset) {
    if (!s || !bytes) {
        set_error("rsd_scene_export_bvh: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    *bytes = s->bvh_bytes;
    if (tri_offset) *tri_offset = s->tri_offset;
    if (!dst) return RSD_OK;
    if (capacity < s->bvh_bytes) {
        set_error("rsd_scene_export_bvh: capacity below the BVH size");
        return RSD_ERR_INVALID_ARG;
    }
    if (s->bvh_bytes == 0) return RSD_OK;
    RSD_HIP(hipSetDevice(s->dev->hip_device));
    RSD_HIP(hipMemcpy(dst, s->d_nodes, s->bvh_bytes, hipMemcpyDeviceToHost));
    return RSD_OK;
}

extern "C" void rsd_scene_release(rsd_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->dev->hip_device);
    (void)hipFree(s->d_nodes);
    (void)hipFree(s->d_prim_rec);
    rsd::release_sd_workspaces(s);
    (void)hipFree(s->d_alpha);
    (void)hipFree(s->d_entry);
    (void)hipFree(s->d_rtao_table);
    (void)hipFree(s->d_dyn);
    (void)hipFree(s->dyn.prev_positions);
    (void)hipFree(s->d_rig);
    (void)hipFree(s->d_morph);
    delete s;
}

// ---- Camera::calculateCameraParameters, Camera.cpp:99-185 (preserveHeight), with
//      MatrixMath.h:686-712 (RightHanded look-at) and VectorMath.h:1731 normalize.
namespace {
struct v3 { float x, y, z; };
inline float dot3(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline v3 cross3(v3 a, v3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline v3 norm3(v3 v) {
    float inv = 1.0f / std::sqrt(dot3(v, v));
    return {v.x * inv, v.y * inv, v.z * inv};
}
}  // namespace

extern "C" rsd_status rsd_camera_look_at(const float pos[3], const float target[3], const float up[3],
                                         float focal_length, float frame_height, float aspect_ratio, float near_z,
                                         float far_z, float focal_distance, rsd_camera* c) {
    if (!pos || !target || !up || !c) {
        set_error("rsd_camera_look_at: null argument");
        return RSD_ERR_INVALID_ARG;
    }
    std::memset(c, 0, sizeof(*c));
    const v3 P{pos[0], pos[1], pos[2]}, T{target[0], target[1], target[2]}, Up{up[0], up[1], up[2]};
    for (int i = 0; i < 3; ++i) c->posW[i] = pos[i];
    c->nearZ = near_z;
    c->farZ = far_z;
    c->focalLength = focal_length;
    c->frameHeight = frame_height;
    c->aspectRatio = aspect_ratio;
    c->frameWidth = frame_height * aspect_ratio;
    const float fovY = focal_length == 0.0f ? 0.0f : 2.0f * std::atan(0.5f * frame_height / focal_length);
    const v3 f = norm3({P.x - T.x, P.y - T.y, P.z - T.z});
    const v3 r = norm3(cross3(Up, f));
    const v3 u = cross3(f, r);
    float* m = c->viewMat;
    m[0] = r.x; m[1] = r.y; m[2] = r.z; m[3] = -dot3(r, P);
    m[4] = u.x; m[5] = u.y; m[6] = u.z; m[7] = -dot3(u, P);
    m[8] = f.x; m[9] = f.y; m[10] = f.z; m[11] = -dot3(f, P);
    m[15] = 1.0f;
    const v3 w = norm3({T.x - P.x, T.y - P.y, T.z - P.z});
    const v3 W{w.x * focal_distance, w.y * focal_distance, w.z * focal_distance};
    const v3 cu = norm3(cross3(W, Up));
    const v3 cv = norm3(cross3(cu, W));
    const float ulen = focal_distance * std::tan(fovY * 0.5f) * aspect_ratio;
    const float vlen = focal_distance * std::tan(fovY * 0.5f);
    c->W[0] = W.x; c->W[1] = W.y; c->W[2] = W.z;
    c->U[0] = cu.x * ulen; c->U[1] = cu.y * ulen; c->U[2] = cu.z * ulen;
    c->V[0] = cv.x * vlen; c->V[1] = cv.y * vlen; c->V[2] = cv.z * vlen;
    return RSD_OK;
}

// SVAO::compile (SVAO.cpp:143-150), getStochMapSize (:700-716), getExtraGuardBand (:718-723)
extern "C" rsd_status rsd_svao_make_vao_data(uint32_t fb_w, uint32_t fb_h, uint32_t divisor, int32_t sd_guard_px,
                                             float radius, float exponent, float thickness, rsd_vao_data* out,
                                             uint32_t* sd_w, uint32_t* sd_h) {
    if (!out || fb_w == 0 || fb_h == 0 || divisor == 0 || sd_guard_px < 0) {
        set_error("rsd_svao_make_vao_data: invalid argument");
        return RSD_ERR_INVALID_ARG;
    }
    rsd_vao_data d{};
    d.resolution[0] = (float)fb_w;
    d.resolution[1] = (float)fb_h;
    d.invResolution[0] = 1.0f / d.resolution[0];
    d.invResolution[1] = 1.0f / d.resolution[1];
    d.sdGuard = sd_guard_px / (int32_t)divisor;
    const uint32_t lw = divisor > 1 ? (fb_w + divisor - 1) / divisor : fb_w;
    const uint32_t lh = divisor > 1 ? (fb_h + divisor - 1) / divisor : fb_h;
    d.lowResolution[0] = (float)lw;
    d.lowResolution[1] = (float)lh;
    d.noiseScale[0] = d.resolution[0] / 4.0f;
    d.noiseScale[1] = d.resolution[1] / 4.0f;
    d.radius = radius;
    d.exponent = exponent;
    d.thickness = thickness;
    d.ssRadiusCutoff = 6.0f;   // VAOData.slang:43
    d.ssMaxRadius = 512.0f;    // VAOData.slang:44
    *out = d;
    if (sd_w) *sd_w = lw + 2u * (uint32_t)d.sdGuard;
    if (sd_h) *sd_h = lh + 2u * (uint32_t)d.sdGuard;
    return RSD_OK;
}
