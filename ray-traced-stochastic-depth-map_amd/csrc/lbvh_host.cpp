// lbvh_host.cpp -- the LBVH of lbvh.h on the host (rsd_bvh_build_lbvh): the byte-exact statement of what
// rsd_scene_rebuild_bvh leaves on the device.  Single-threaded; follows the kernels of lbvh.hip step by step
// (keys, sort, one Karras node per internal node, depths up the parent chain, wide nodes numbered by a sort of
// (wide depth, first position)), then fills the boxes with the host refit.
#include "lbvh.h"

#include <algorithm>
#include <cstring>

namespace rsd {

LbvhResult lbvh_build_host(const float* positions, uint32_t nv, const uint32_t* indices, uint32_t nt,
                           const uint32_t* flags, std::vector<uint32_t>& out) {
    LbvhResult res;
    const uint32_t* pos = reinterpret_cast<const uint32_t*>(positions);
    // scene box over the referenced vertices
    RefitBox box;
    refit_box_clear(box);
    for (size_t c = 0; c < 3 * (size_t)nt; ++c) {
        const uint32_t v = indices[c];
        if (v >= nv) continue;
        for (int k = 0; k < 3; ++k) {
            const uint32_t key = refit_key(pos[3 * (size_t)v + k]);
            box.lo[k] = key < box.lo[k] ? key : box.lo[k];
            box.hi[k] = key > box.hi[k] ? key : box.hi[k];
        }
    }
    std::vector<uint64_t> keys(nt);
    for (uint32_t t = 0; t < nt; ++t) keys[t] = lbvh_key(t, indices, pos, nv, box);
    std::sort(keys.begin(), keys.end());

    // binary tree, wide nodes and their numbers
    const uint32_t ni = nt > kLbvhLeaf ? nt - 1 : 0;  // internal binary nodes that matter: none for a leaf root
    std::vector<uint32_t> first(ni), last(ni), split(ni), parent(ni, 0xffffffffu), widx(ni, 0xffffffffu);
    for (uint32_t i = 0; i < ni; ++i) {
        const LbvhNode n = lbvh_karras(keys.data(), nt, i);
        first[i] = n.first;
        last[i] = n.last;
        split[i] = n.split;
        if (n.first != n.split) parent[n.split] = i;
        if (n.split + 1 != n.last) parent[n.split + 1] = i;
    }
    std::vector<std::pair<uint64_t, uint32_t>> wide;  // (number key, binary node)
    for (uint32_t i = 0; i < ni; ++i) {
        uint32_t depth = 0;
        for (uint32_t p = parent[i]; p != 0xffffffffu; p = parent[p]) ++depth;
        res.max_depth = std::max(res.max_depth, depth + 1);  // its children lie one level down
        if (depth % 2 == 0 && last[i] - first[i] + 1 > kLbvhLeaf) wide.push_back({lbvh_wide_key(depth / 2, first[i]), i});
    }
    std::sort(wide.begin(), wide.end());
    for (uint32_t w = 0; w < wide.size(); ++w) widx[wide[w].second] = w;
    const uint32_t nn = ni ? (uint32_t)wide.size() : 1u;
    res.node_count = nn;
    res.wide_depth = ni ? (uint32_t)(wide.back().first >> 32) + 1 : 1u;

    out.assign(32 * (size_t)nn + 12 * (size_t)nt + 48, 0u);
    for (uint32_t n = 0; n < nn; ++n)
        for (uint32_t k = 0; k < 4; ++k) out[32 * (size_t)n + 24 + k] = kRefitEmptyRef;
    if (!ni) {
        if (nt) {
            out[24] = 0;
            out[28] = nt;
            res.leaf_slots = 1;
        }
    } else {
        for (uint32_t w = 0; w < nn; ++w) {
            const LbvhSlots s = lbvh_slots(first.data(), last.data(), split.data(), wide[w].second);
            for (uint32_t k = 0; k < s.n; ++k) {
                const uint32_t size = s.b[k] - s.a[k] + 1;
                out[32 * (size_t)w + 24 + k] = size > kLbvhLeaf ? widx[s.id[k]] : s.a[k];
                out[32 * (size_t)w + 28 + k] = size > kLbvhLeaf ? 0u : size;
                res.leaf_slots += size <= kLbvhLeaf;
            }
        }
    }
    for (uint32_t r = 0; r < nt; ++r) {
        const uint32_t prim = (uint32_t)(keys[r] & 0xffffffffu);
        out[32 * (size_t)nn + 12 * (size_t)r + 3] = prim;
        out[32 * (size_t)nn + 12 * (size_t)r + 7] = flags ? flags[prim] : 0u;
    }
    refit_host(out.data(), nn, indices, nt, positions);
    return res;
}

}  // namespace rsd
