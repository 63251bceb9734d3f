// lbvh.h -- the definition of the tree rsd_scene_rebuild_bvh builds on the GPU (lbvh.hip) and
// rsd_bvh_build_lbvh builds on the host (lbvh_host.cpp), shared by both so that they produce the same bytes
// (DESIGN.md 4 "Rebuilding topology on the GPU").  Boxes are not defined here: the tree is topology and record
// order, and bvh_refit.h's rule fills in every box.
//
//   scene box   per axis the min / max, by bvh_refit.h's integer keys, over the vertices triangles reference
//   code        per triangle and axis: q = lbvh_quantise(lo, hi, slo, shi) of the triangle's own tight box
//               [lo, hi] inside the scene box [slo, shi]; code = interleave(qx, qy, qz), x in the highest bit
//   key         code << 32 | prim; the keys are distinct, so their ascending order is unique.  Record r holds
//               the triangle key[r] & 0xffffffff.
//   binary tree Karras 2012 over the sorted keys: the node of a range [a, b] splits at the highest bit in which
//               key[a] and key[b] differ; the left part ends at the last position that agrees with key[a] above
//               that bit (lbvh_karras: internal node i covers a range one of whose ends is i)
//   wide nodes  a range of more than 4 triangles at an even binary depth.  It splits once, and each half of more
//               than 4 triangles once more: 2 to 4 child ranges, left to right in slots 0 and up (lbvh_slots).
//               A child range of at most 4 triangles is a leaf slot, a larger one an inner slot.  nt <= 4: one
//               node with one leaf slot (none for nt = 0).
//   numbering   wide nodes ascending by (wide depth, first position), the root 0
//
// Float mode: the only arithmetic on coordinates is lbvh_quantise, which compares through the integer keys,
// widens to double by integer operations and then uses five double operations, each rounded on its own (the
// library is compiled with -ffp-contract=off; double division is correctly rounded on the host and on gfx950
// whatever the float32 options).  Float32 denormal flushing and fast-math flags do not reach it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bvh_refit.h"

namespace rsd {

constexpr uint32_t kLbvhLeaf = 4;          // triangles a leaf slot holds at most (bvh_build.h kBvhMaxLeaf)
constexpr uint32_t kLbvhCodeBits = 30;     // 10 bits per axis
// Depth.  Keys differ only in their low 30 + ceil(log2 nt) bits, every binary split consumes at least one of
// them, and wide nodes sit on every second binary level: a path holds at most (30 + ceil(log2 nt)) / 2 + 1 wide
// nodes.  A walk pushes at most 3 entries per wide node it descends through (bvh_traverse.h), so its stack of
// kStackTotal = 96 entries holds 32 levels: ceil(log2 nt) <= 33.  Primitive ids are 32 bits and an upload
// already refuses 2^30 triangles and more, which is therefore the limit that binds (depth <= 31).
constexpr uint32_t kLbvhStackEntries = 96;  // bvh_traverse.h kStackTotal (lbvh.hip asserts the two agree)
constexpr uint32_t kLbvhMaxWideDepth = kLbvhStackEntries / 3;
constexpr uint32_t lbvh_ceil_log2(uint64_t n) {
    uint32_t l = 0;
    while (l < 63 && (1ull << l) < n) ++l;
    return l;
}
constexpr uint32_t lbvh_depth_bound(uint64_t nt) { return (kLbvhCodeBits + lbvh_ceil_log2(nt)) / 2 + 1; }
constexpr uint64_t kLbvhMaxTriangles = (1ull << 30) - 1;  // rsd_scene_upload's own limit
static_assert(lbvh_depth_bound(kLbvhMaxTriangles) <= kLbvhMaxWideDepth, "the deepest LBVH fits the walks' stacks");
static_assert(lbvh_depth_bound(1ull << 33) <= kLbvhMaxWideDepth && lbvh_depth_bound((1ull << 33) + 1) > kLbvhMaxWideDepth,
              "2^33 triangles is where the stack bound itself would bind");

// the value of a finite float32 given by its bits, as a double, by integer operations alone
RSD_HD double lbvh_value(uint32_t bits) {
    const uint32_t e = (bits >> 23) & 0xffu, m = bits & 0x7fffffu;
    double v;
    if (e == 0u) {
        v = (double)(int32_t)m * 0x1p-149;  // zeros and denormals: m 2^-149, exact
    } else {
        const uint64_t d = ((uint64_t)(e + 896u) << 52) | ((uint64_t)m << 29);  // rebias 127 -> 1023
        __builtin_memcpy(&v, &d, 8);
    }
    return (bits & 0x80000000u) ? -v : v;
}
RSD_HD bool lbvh_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// One axis of a code: the midpoint of [lo, hi] (a triangle's tight box) quantised to 10 bits inside [slo, shi]
// (the scene box); all four are float32 bit patterns.  0 for an axis of zero extent or a non-finite value.
//   q = ((lo + hi) * 0.5 - slo) / (shi - slo) * 1024, in double, each operation rounded on its own;
//   the code is trunc(q) clamped to [0, 1023]
RSD_HD uint32_t lbvh_quantise(uint32_t lo, uint32_t hi, uint32_t slo, uint32_t shi) {
    if (!lbvh_finite(lo) || !lbvh_finite(hi) || !lbvh_finite(slo) || !lbvh_finite(shi)) return 0u;
    const double s0 = lbvh_value(slo);
    const double ext = lbvh_value(shi) - s0;
    if (!(ext > 0.0)) return 0u;
    const double sum = lbvh_value(lo) + lbvh_value(hi);
    const double mid = sum * 0.5;
    const double rel = mid - s0;
    const double q = rel / ext * 1024.0;
    if (!(q >= 0.0)) return 0u;
    if (q >= 1023.0) return 1023u;
    return (uint32_t)q;
}

// 10 bits -> every third bit of 30
RSD_HD uint32_t lbvh_spread(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
RSD_HD uint32_t lbvh_morton(uint32_t qx, uint32_t qy, uint32_t qz) {
    return lbvh_spread(qx) << 2 | lbvh_spread(qy) << 1 | lbvh_spread(qz);
}

// The key of triangle `prim`: ind / pos are the scene's index buffer and positions (as words), box the scene box
// as keys.  A vertex index outside [0, nv) is skipped (uploads check them; the kernels never read out of bounds).
RSD_HD uint64_t lbvh_key(uint32_t prim, const uint32_t* ind, const uint32_t* pos, uint32_t nv, const RefitBox& box) {
    RefitBox t;
    refit_box_clear(t);
    for (int j = 0; j < 3; ++j) {
        const uint32_t v = ind[3 * (size_t)prim + j];
        if (v >= nv) continue;
        for (int k = 0; k < 3; ++k) {
            const uint32_t key = refit_key(pos[3 * (size_t)v + k]);
            t.lo[k] = key < t.lo[k] ? key : t.lo[k];
            t.hi[k] = key > t.hi[k] ? key : t.hi[k];
        }
    }
    uint32_t q[3];
    for (int k = 0; k < 3; ++k)
        q[k] = t.lo[k] > t.hi[k] ? 0u
                                 : lbvh_quantise(refit_unkey(t.lo[k]), refit_unkey(t.hi[k]), refit_unkey(box.lo[k]),
                                                 refit_unkey(box.hi[k]));
    return (uint64_t)lbvh_morton(q[0], q[1], q[2]) << 32 | prim;
}

// common leading bits of keys i and j of `n` sorted distinct keys, -1 for j outside [0, n)
RSD_HD int lbvh_delta(const uint64_t* keys, int64_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(keys[i] ^ keys[j]);
}

// Internal node i (0 <= i < n - 1, n >= 2) of Karras's binary radix tree over n sorted distinct keys: its range
// [first, last] and the last position `split` of its left part.  The left child is internal node `split` unless
// first == split (a leaf), the right child internal node split + 1 unless split + 1 == last.  Node 0 is the root.
struct LbvhNode {
    uint32_t first, last, split;
};
RSD_HD LbvhNode lbvh_karras(const uint64_t* keys, uint32_t n32, uint32_t i32) {
    const int64_t n = n32, i = i32;
    const int64_t d = lbvh_delta(keys, n, i, i + 1) > lbvh_delta(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = lbvh_delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = lbvh_delta(keys, n, i, j);
    int64_t s = 0;
    for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t split = i + s * d + (d < 0 ? -1 : 0);
    LbvhNode out;
    out.first = (uint32_t)(d > 0 ? i : j);
    out.last = (uint32_t)(d > 0 ? j : i);
    out.split = (uint32_t)split;
    return out;
}

// The child ranges of the wide node at internal binary node i, left to right: n of them (2 to 4), range
// [a[k], b[k]], whose binary node (when it holds more than one triangle) is internal node id[k].
// first / last / split: lbvh_karras's results per internal node.
struct LbvhSlots {
    uint32_t n;
    uint32_t a[4], b[4], id[4];
};
RSD_HD LbvhSlots lbvh_slots(const uint32_t* first, const uint32_t* last, const uint32_t* split, uint32_t i) {
    LbvhSlots s;
    s.n = 0;
    const uint32_t ha[2] = {first[i], split[i] + 1u}, hb[2] = {split[i], last[i]}, hid[2] = {split[i], split[i] + 1u};
    for (int h = 0; h < 2; ++h) {
        if (hb[h] - ha[h] + 1u > kLbvhLeaf) {
            const uint32_t sp = split[hid[h]];
            s.a[s.n] = ha[h]; s.b[s.n] = sp; s.id[s.n] = sp; ++s.n;
            s.a[s.n] = sp + 1u; s.b[s.n] = hb[h]; s.id[s.n] = sp + 1u; ++s.n;
        } else {
            s.a[s.n] = ha[h]; s.b[s.n] = hb[h]; s.id[s.n] = hid[h]; ++s.n;
        }
    }
    return s;
}

// the sort key of a wide node's number: (wide depth, first position)
RSD_HD uint64_t lbvh_wide_key(uint32_t level, uint32_t first) { return (uint64_t)level << 32 | first; }

// What the host builder returns besides the bytes
struct LbvhResult {
    uint32_t node_count = 0, wide_depth = 0, max_depth = 0, leaf_slots = 0;
};
// The tree of the definition above on the host: `out` receives node_count x 32 node words, then nt x 12 record
// words, then 48 zero words -- rsd_bvh_build's layout.  flags may be null.  Single-threaded.
LbvhResult lbvh_build_host(const float* positions, uint32_t nv, const uint32_t* indices, uint32_t nt,
                           const uint32_t* flags, std::vector<uint32_t>& out);

}  // namespace rsd
