// check_lbvh.cpp -- host check of the LBVH builder (csrc/lbvh.h, lbvh_host.cpp), meant to run under
// -fsanitize=address,undefined (tests/test_lbvh.py builds it so).
//
// The builder runs on the shapes at which a Morton-code tree degenerates: no triangle, 1, 4, 5 and 9 triangles,
// coincident triangles (every code equal), a planar and a collinear scene (axes of zero extent), denormal and huge
// coordinates, an infinite coordinate (that axis quantises to 0), shared vertices, and random soups of a few
// thousand triangles.  Checked for each: the size and layout of the bytes; refit_topology accepts the nodes (a
// parent's index below its children's, one parent each, leaf ranges inside the records); every primitive has exactly
// one record and carries its flags; every record lies under exactly one leaf slot of at most 4; the records are in
// key order, the keys recomputed here with lbvh_key; the depth the builder reports is the tree's and within
// lbvh_depth_bound; a second build gives the same bytes.  The quantiser is checked at the edges of its range.
// Prints "failures N" (0 expected).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bvh_refit.h"
#include "lbvh.h"

using namespace rsd;

namespace {
int failures = 0;
void expect(bool ok, const char* what, const char* scene = "") {
    if (!ok) {
        ++failures;
        std::printf("FAIL %s %s\n", what, scene);
    }
}
uint32_t fbits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

void check_quantise() {
    const uint32_t z = fbits(0.0f), one = fbits(1.0f), half = fbits(0.5f);
    expect(lbvh_quantise(z, z, z, one) == 0, "q(0)");
    expect(lbvh_quantise(one, one, z, one) == 1023, "q(1) clamps");
    expect(lbvh_quantise(half, half, z, one) == 512, "q(0.5)");
    expect(lbvh_quantise(z, one, z, one) == 512, "midpoint");
    expect(lbvh_quantise(half, half, half, half) == 0, "zero extent");
    expect(lbvh_quantise(half, fbits(INFINITY), z, one) == 0, "infinite bound");
    expect(lbvh_quantise(half, half, z, fbits(std::nanf(""))) == 0, "NaN scene box");
    expect(lbvh_quantise(fbits(-2.0f), fbits(-2.0f), z, one) == 0, "below the box");
    expect(lbvh_quantise(fbits(1e-45f), fbits(1e-45f), fbits(-1e-45f), fbits(1e-45f)) == 1023, "denormal box");
    expect(lbvh_quantise(z, z, fbits(-1e-45f), fbits(1e-45f)) == 512, "denormal midpoint");
    expect(lbvh_quantise(fbits(3e38f), fbits(3e38f), fbits(-3e38f), fbits(3e38f)) == 1023, "huge box: no overflow in double");
    const float vals[] = {0.0f, -0.0f, 1.0f, -1.5f, 1e-45f, -1e-40f, 1.17549435e-38f, 3.4028235e38f, 0.1f};
    for (float v : vals) expect(lbvh_value(fbits(v)) == (double)v, "lbvh_value");
    expect(lbvh_morton(1023, 0, 0) == 0x24924924u && lbvh_morton(0, 1023, 0) == 0x12492492u &&
               lbvh_morton(0, 0, 1023) == 0x09249249u && lbvh_morton(1, 0, 0) == 4u,
           "morton");
}

void check_scene(const char* name, const std::vector<float>& pos, const std::vector<uint32_t>& ind) {
    const uint32_t nt = (uint32_t)(ind.size() / 3), nv = (uint32_t)(pos.size() / 3);
    std::vector<uint32_t> flags(nt);
    for (uint32_t t = 0; t < nt; ++t) flags[t] = (t * 2654435761u) >> 30;
    std::vector<uint32_t> w, again;
    const LbvhResult res = lbvh_build_host(pos.data(), nv, ind.data(), nt, flags.data(), w);
    lbvh_build_host(pos.data(), nv, ind.data(), nt, flags.data(), again);
    expect(w == again, "deterministic", name);
    const uint32_t nn = res.node_count;
    expect(nn >= 1 && w.size() == 32 * (size_t)nn + 12 * (size_t)nt + 48, "layout", name);
    if (w.size() != 32 * (size_t)nn + 12 * (size_t)nt + 48) return;
    for (size_t i = w.size() - 48; i < w.size(); ++i) expect(w[i] == 0, "pad", name);
    std::vector<uint32_t> parent(nn), inner(nn);
    expect(refit_topology(w.data(), nn, nt, parent.data(), inner.data()), "topology", name);
    // records: one per primitive, in key order
    RefitBox box;
    refit_box_clear(box);
    for (uint32_t v : ind)
        for (int k = 0; k < 3; ++k) {
            const uint32_t key = refit_key(fbits(pos[3 * (size_t)v + k]));
            box.lo[k] = key < box.lo[k] ? key : box.lo[k];
            box.hi[k] = key > box.hi[k] ? key : box.hi[k];
        }
    std::vector<uint8_t> seen(nt, 0);
    uint64_t prevKey = 0;
    for (uint32_t r = 0; r < nt; ++r) {
        const uint32_t* rec = &w[32 * (size_t)nn + 12 * (size_t)r];
        const uint32_t prim = rec[3];
        expect(prim < nt && !seen[prim < nt ? prim : 0], "one record per primitive", name);
        if (prim >= nt) return;
        seen[prim] = 1;
        expect(rec[7] == flags[prim] && rec[11] == 0, "flags", name);
        for (int j = 0; j < 3; ++j)
            expect(std::memcmp(rec + 4 * j, &pos[3 * (size_t)ind[3 * (size_t)prim + j]], 12) == 0, "positions", name);
        const uint64_t key = lbvh_key(prim, ind.data(), reinterpret_cast<const uint32_t*>(pos.data()), nv, box);
        expect(r == 0 || key > prevKey, "key order", name);
        prevKey = key;
    }
    // leaves cover every record once; depth
    std::vector<uint32_t> covered(nt, 0), depth(nn, 0);
    uint32_t deepest = 0, leafSlots = 0;
    depth[0] = 1;
    for (uint32_t n = 0; n < nn; ++n) {
        deepest = depth[n] > deepest ? depth[n] : deepest;
        uint32_t usedSlots = 0;
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t ref = w[32 * (size_t)n + 24 + i], cnt = w[32 * (size_t)n + 28 + i];
            if (cnt) {
                ++leafSlots;
                expect(cnt <= kLbvhLeaf && ref + cnt <= nt, "leaf slot", name);
                for (uint32_t t = ref; t < ref + cnt && t < nt; ++t) ++covered[t];
            } else if (ref != kRefitEmptyRef && ref < nn) {
                depth[ref] = depth[n] + 1;
            }
            if (cnt || ref != kRefitEmptyRef) {
                expect(usedSlots == i, "slots fill from 0 up", name);
                ++usedSlots;
            }
        }
        expect(nt <= kLbvhLeaf || usedSlots >= 2, "a wide node has 2 to 4 children", name);
    }
    for (uint32_t t = 0; t < nt; ++t) expect(covered[t] == 1, "covered once", name);
    expect(deepest == res.wide_depth && res.wide_depth <= lbvh_depth_bound(nt), "depth", name);
    expect(leafSlots == res.leaf_slots, "leaf slots", name);
}

void soup(uint32_t nt, float spread, uint32_t seed, std::vector<float>& pos, std::vector<uint32_t>& ind) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    pos.clear();
    ind.clear();
    for (uint32_t t = 0; t < nt; ++t) {
        const float c[3] = {spread * U(rng), spread * U(rng), spread * U(rng)};
        for (int j = 0; j < 3; ++j) {
            for (int k = 0; k < 3; ++k) pos.push_back(c[k] + 0.3f * U(rng));
            ind.push_back(3 * t + j);
        }
    }
}
}  // namespace

int main() {
    check_quantise();
    std::vector<float> pos;
    std::vector<uint32_t> ind;
    check_scene("empty", pos, ind);
    for (uint32_t nt : {1u, 2u, 4u, 5u, 9u, 300u, 6000u}) {
        soup(nt, nt > 100 ? 10.0f : 1.0f, nt, pos, ind);
        if (nt > 4) {  // shared and repeated vertices
            ind[3] = ind[0];
            ind[7] = ind[2];
        }
        char name[32];
        std::snprintf(name, sizeof(name), "soup_%u", nt);
        check_scene(name, pos, ind);
    }
    {  // coincident: every code equal, the primitive id alone shapes the tree
        pos = {-1, -1, 0, 1, -1, 0, 0, 1, 0.5f};
        ind.clear();
        for (int t = 0; t < 37; ++t) ind.insert(ind.end(), {0u, 1u, 2u});
        check_scene("coincident", pos, ind);
        ind.resize(3 * 5);
        check_scene("coincident_5", pos, ind);
    }
    {  // planar (z constant) and collinear (y and z constant)
        soup(500, 5.0f, 21, pos, ind);
        for (size_t v = 0; v < pos.size() / 3; ++v) pos[3 * v + 2] = 0.25f;
        check_scene("planar", pos, ind);
        for (size_t v = 0; v < pos.size() / 3; ++v) pos[3 * v + 1] = -3.0f;
        check_scene("collinear", pos, ind);
        for (size_t v = 0; v < pos.size() / 3; ++v) pos[3 * v] = 7.0f;
        check_scene("one_point", pos, ind);
    }
    {  // denormal coordinates on both sides of zero, huge ones, and an infinite one
        soup(400, 3.0f, 22, pos, ind);
        std::vector<float> p = pos;
        for (float& v : p) v = (float)((double)v * 1e-41);
        p[0] = 0.0f;
        p[1] = -0.0f;
        check_scene("denormal", p, ind);
        p = pos;
        for (float& v : p) v *= 1e37f;
        check_scene("huge", p, ind);
        p = pos;
        p[4] = std::numeric_limits<float>::infinity();
        check_scene("infinite", p, ind);
    }
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
