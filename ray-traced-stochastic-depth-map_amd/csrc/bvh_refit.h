// bvh_refit.h -- the box rule of a BVH refit, shared by the host refit (bvh_refit_host.cpp) and the
// refit kernels (bvh_refit.hip), so that both produce the same bytes.
//
// A refit keeps the tree (every ref / cnt word, every record's prim / flags word) and rewrites
//   - the triangle records' twelve position floats from the index buffer and the new positions,
//   - every child slot's box: the TIGHT min / max over all vertices under that child, moved two
//     floats outward per bound -- what bvh_build.cpp's collapse stores (nextafter twice).
// Tight boxes, not stored ones, propagate upward (a parent's slot is two floats outside the
// union of the tight boxes below it, not four).
//
// Nothing here uses float arithmetic or float comparisons: bounds are compared through an
// order-preserving integer key and stepped on the bit pattern, so the result does not depend
// on the float mode (denormal flushing, fast-math) of whoever compiles it.  The key orders
// -0 below +0, where a float compare calls them equal; both zeros step to the same
// neighbours, so the stored bytes do not depend on which one a min / max kept.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RSD_HD __host__ __device__ inline
#else
#define RSD_HD inline
#endif

namespace rsd {

// float bits -> unsigned key with the order of the floats (-inf lowest, +inf highest below the
// positive NaNs), and back
RSD_HD uint32_t refit_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
RSD_HD uint32_t refit_unkey(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// std::nextafter(v, -INFINITY) on the bit pattern: zeros of either sign step to the smallest
// negative denormal, -inf and NaNs stay
RSD_HD uint32_t refit_next_down(uint32_t b) {
    const uint32_t mag = b & 0x7fffffffu;
    if (mag > 0x7f800000u) return b;          // NaN
    if (mag == 0u) return 0x80000001u;        // +-0 -> -denorm_min
    if (b & 0x80000000u) return b == 0xff800000u ? b : b + 1u;  // negative: away from zero
    return b - 1u;                            // positive: towards zero (+inf -> FLT_MAX)
}
// std::nextafter(v, +INFINITY): -denorm_min steps to -0, which steps to +denorm_min
RSD_HD uint32_t refit_next_up(uint32_t b) {
    const uint32_t mag = b & 0x7fffffffu;
    if (mag > 0x7f800000u) return b;
    if (mag == 0u) return 0x00000001u;
    if (b & 0x80000000u) return b - 1u;       // negative: towards zero (-inf -> -FLT_MAX)
    return b == 0x7f800000u ? b : b + 1u;
}
RSD_HD uint32_t refit_pad_lo(uint32_t b) { return refit_next_down(refit_next_down(b)); }
RSD_HD uint32_t refit_pad_hi(uint32_t b) { return refit_next_up(refit_next_up(b)); }

// A tight box as keys: lo[3] then hi[3].  Empty: lo = 0xffffffff, hi = 0.
struct RefitBox {
    uint32_t lo[3], hi[3];
};
RSD_HD void refit_box_clear(RefitBox& b) {
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = 0xffffffffu;
        b.hi[k] = 0u;
    }
}
RSD_HD void refit_box_grow(RefitBox& b, const RefitBox& o) {
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = o.lo[k] < b.lo[k] ? o.lo[k] : b.lo[k];
        b.hi[k] = o.hi[k] > b.hi[k] ? o.hi[k] : b.hi[k];
    }
}
// the nine position words of `cnt` consecutive triangle records starting at `rec` (12 words each,
// positions at words 0-2, 4-6, 8-10)
RSD_HD void refit_box_grow_records(RefitBox& b, const uint32_t* rec, uint32_t cnt) {
    for (uint32_t t = 0; t < cnt; ++t)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) {
                const uint32_t key = refit_key(rec[12 * (size_t)t + 4 * j + k]);
                b.lo[k] = key < b.lo[k] ? key : b.lo[k];
                b.hi[k] = key > b.hi[k] ? key : b.hi[k];
            }
}
// the padded box of tight box `b` into slot `slot` of the wide node at `node` (32 words, SoA:
// lo.x[4] hi.x[4] lo.y[4] hi.y[4] lo.z[4] hi.z[4] ref[4] cnt[4])
RSD_HD void refit_store_slot(uint32_t* node, uint32_t slot, const RefitBox& b) {
    for (int k = 0; k < 3; ++k) {
        node[8 * k + slot] = refit_pad_lo(refit_unkey(b.lo[k]));
        node[8 * k + 4 + slot] = refit_pad_hi(refit_unkey(b.hi[k]));
    }
}

constexpr uint32_t kRefitNoParent = 0xffffffffu;  // the root's parent word
constexpr uint32_t kRefitEmptyRef = 0xffffffffu;  // ref of an empty slot (its cnt is 0)

// Topology of a flattened tree (FlatBvh::nodes as words): per wide node its parent `node << 2 | slot`
// (the root: kRefitNoParent) and its count of inner children.  Returns false if the tree is not one
// librsd built: a child reference that leaves the tree or does not lie above its parent's index, a node
// with two parents or none, a leaf whose records leave [0, record_count).
bool refit_topology(const uint32_t* nodes, uint32_t node_count, uint32_t record_count, uint32_t* parent,
                    uint32_t* inner);

// The refit on the host: rewrites the records' positions and every slot box of `bvh` (the bytes of
// rsd_bvh_build / rsd_scene_export_bvh: node_count wide nodes, then nt records) in place.
void refit_host(uint32_t* bvh, uint32_t node_count, const uint32_t* indices, uint32_t nt, const float* positions);

}  // namespace rsd
