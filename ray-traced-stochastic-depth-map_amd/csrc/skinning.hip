// skinning.hip -- animated scenes: pose the vertices a rig names from a small table of 3x4 matrices, in stream
// order (rsd_scene_update_pose).  The reference's Skinning.slang, one thread per dynamic vertex, reduced to
// what the traces read: positions.  Rigid node animation and 4-influence linear-blend skinning are the same
// kernel; a rigid vertex is the rig entry ids (m, 0, 0, 0), weights (1, 0, 0, 0).
//
// One lane per animated vertex: it reads its vertex id (4 B), four matrix ids (16 B), four weights (16 B) and
// its rest position (12 B), blends the four matrices, transforms, and stores three floats (12 B) into the
// scene's position copy at that vertex -- 60 B of stream traffic per vertex, the stores scattered by the
// vertex id.  Vertices outside the rig are neither read nor written.  The launches of a refit
// (bvh_refit.hip) follow on the same stream.
//
// The arithmetic is librsd's definition (rsd.h rsd_scene_update_pose, DESIGN.md 4 "Animated scenes") and is
// stated a second time only in tests/skinning_checker.py: all four slots are always evaluated, a weight of 0
// included, every product and sum is rounded on its own (this file is compiled with -ffp-contract=off like
// every exact kernel), nothing is normalised and there is no shortcut for rigid vertices.
//
// Morph targets (rsd_scene_attach_morph, pose_kernel<*, true>): before the blend a lane reads its two CSR offsets
// (8 B) and walks its entries in ascending order, one 16-byte record {weight id, dx, dy, dz} each, adding
// w[id] * delta to the rest position -- product rounded, then sum, every entry evaluated.  The weights are a small
// table every lane gathers from (it stays in the vector L1 / L2).  So a vertex of k entries streams 60 + 8 + 16 k
// bytes; the entries of neighbouring lanes are neighbours in memory (CSR), and lanes of one wave with different
// entry counts idle until the longest has finished.  The morphed position lives in registers only: there is no
// second launch and no scratch.  Without a table the kernel is pose_kernel<*, false>: the code of before.
//
// The matrix table: each lane reads its four matrices with 16-byte loads through the vector L1 (pose_kernel
// <false>), or the workgroup first stages the whole table in LDS (pose_kernel<true>, tables of at most
// kPoseLdsMatrices).  Which one runs: pose_enqueue below; the measurement behind it is DESIGN.md's table
// (tools/skinning_time.py).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "rsd_internal.h"

namespace rsd {
namespace {

constexpr int kPoseBlock = 256;
constexpr uint32_t kPoseLdsMatrices = 256;  // 12 KiB of LDS

struct Row4 {
    float v[4];
};

__device__ inline Row4 load_row(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    return Row4{{q.x, q.y, q.z, q.w}};
}

// the morph table as the kernel reads it; all null / 0 for pose_kernel<*, false>
struct MorphArgs {
    const uint32_t* offsets;
    const uint4* entries;
    const float* weights;
    uint32_t weight_count, entry_count;
};

template <bool kLds, bool kMorph>
__global__ __launch_bounds__(kPoseBlock) void pose_kernel(float* __restrict__ pos, uint32_t nv,
                                                          const uint32_t* __restrict__ vertex_ids,
                                                          const uint4* __restrict__ matrix_ids,
                                                          const float4* __restrict__ weights,
                                                          const float* __restrict__ rest,
                                                          const float* __restrict__ matrices, uint32_t matrix_count,
                                                          uint32_t count, MorphArgs morph) {
    __shared__ __attribute__((aligned(16))) float table[kLds ? 12 * kPoseLdsMatrices : 4];
    const float* tab = matrices;
    if (kLds) {
        const uint32_t rows = 3 * matrix_count;  // <= 3 * kPoseLdsMatrices (pose_enqueue)
        for (uint32_t r = threadIdx.x; r < rows; r += kPoseBlock)
            *reinterpret_cast<float4*>(table + 4 * r) = *reinterpret_cast<const float4*>(matrices + 4 * (size_t)r);
        __syncthreads();
        tab = table;
    }
    const uint32_t i = blockIdx.x * kPoseBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t v = vertex_ids[i];
    const uint4 m = matrix_ids[i];
    const float4 w = weights[i];
    // checked on the host at attach; an id outside the scene or the table moves nothing
    if (v >= nv || m.x >= matrix_count || m.y >= matrix_count || m.z >= matrix_count || m.w >= matrix_count) return;
    float x = rest[3 * (size_t)i], y = rest[3 * (size_t)i + 1], z = rest[3 * (size_t)i + 2];
    if (kMorph) {
        // checked on the host at attach; an offset past the entries or an id past the weights adds nothing
        const uint32_t e0 = morph.offsets[i], e1 = min(morph.offsets[i + 1], morph.entry_count);
        for (uint32_t e = e0; e < e1; ++e) {
            const uint4 t = morph.entries[e];
            if (t.x >= morph.weight_count) continue;
            const float wk = morph.weights[t.x];
            x = x + wk * __uint_as_float(t.y);
            y = y + wk * __uint_as_float(t.z);
            z = z + wk * __uint_as_float(t.w);
        }
    }
    for (int r = 0; r < 3; ++r) {
        const Row4 a = load_row(tab + 12 * (size_t)m.x + 4 * r), b = load_row(tab + 12 * (size_t)m.y + 4 * r),
                   c = load_row(tab + 12 * (size_t)m.z + 4 * r), d = load_row(tab + 12 * (size_t)m.w + 4 * r);
        float B[4];
        for (int k = 0; k < 4; ++k) B[k] = ((a.v[k] * w.x + b.v[k] * w.y) + c.v[k] * w.z) + d.v[k] * w.w;
        pos[3 * (size_t)v + r] = ((B[0] * x + B[1] * y) + B[2] * z) + B[3];
    }
}

// RSD_POSE_TABLE = lds | global: the measurement's switch between the two reads of the matrix table
bool pose_table_in_lds(uint32_t matrix_count) {
    if (matrix_count > kPoseLdsMatrices) return false;
    const char* env = std::getenv("RSD_POSE_TABLE");
    return env && std::strcmp(env, "lds") == 0;
}

}  // namespace

rsd_status pose_enqueue(rsd_scene* s, const float* d_matrices, hipStream_t st) {
    const RigData& g = s->rig;
    if (!g.count) return RSD_OK;
    const dim3 grid((g.count + kPoseBlock - 1) / kPoseBlock), block(kPoseBlock);
    const uint4* ids = reinterpret_cast<const uint4*>(g.matrix_ids);
    const float4* wts = reinterpret_cast<const float4*>(g.weights);
    const MorphData& t = s->morph;
    const bool morph = s->d_morph != nullptr && t.count == g.count;
    const MorphArgs ma = morph ? MorphArgs{t.offsets, t.entries, t.weights, t.weight_count, t.entry_count}
                               : MorphArgs{nullptr, nullptr, nullptr, 0, 0};
    const bool lds = pose_table_in_lds(g.matrix_count);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, s->dyn.positions, s->vertex_count, g.vertex_ids, ids, wts,
                           g.rest, d_matrices, g.matrix_count, g.count, ma);
    };
    if (morph)
        lds ? launch(pose_kernel<true, true>) : launch(pose_kernel<false, true>);
    else
        lds ? launch(pose_kernel<true, false>) : launch(pose_kernel<false, false>);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "pose_kernel launch");
}

}  // namespace rsd
