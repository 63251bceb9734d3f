// check_bvh_refit.cpp -- host check of the BVH refit (csrc/bvh_refit.h), meant to run under
// -fsanitize=address,undefined (tests/test_bvh_refit.py builds it so).
//
// Random triangle scenes are built with librsd's own host builder.  Checked: the bit steps against
// std::nextafter at the edges of the float format; a refit to the unchanged positions reproduces the build;
// a refit to moved positions (jitter, a part moved far away, denormal coordinates) equals a restatement with
// float min / max and std::nextafter over each child's subtree, leaves every ref / cnt / prim / flags word
// alone, and the way back reproduces the build; the topology tables describe a tree; a tree built with
// spatial splits has more records than triangles, which is what rsd_bvh_refit refuses.
// Prints "failures N" (0 expected).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bvh_build.h"
#include "bvh_refit.h"

using namespace rsd;

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        std::printf("FAIL %s\n", what);
    }
}
uint32_t fbits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
float bitsf(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

std::vector<uint32_t> flatten(const FlatBvh& b) {
    std::vector<uint32_t> w(b.nodes.size() + b.tris.size() + 48, 0u);
    std::memcpy(w.data(), b.nodes.data(), b.nodes.size() * 4);
    if (!b.tris.empty()) std::memcpy(w.data() + b.nodes.size(), b.tris.data(), b.tris.size() * 4);
    return w;
}

struct FBox {
    float lo[3], hi[3];
};
// float restatement: the tight box under node n, writing every slot of the subtree into `w`
FBox restate(std::vector<uint32_t>& w, uint32_t nn, uint32_t n) {
    const float inf = std::numeric_limits<float>::infinity();
    FBox all{{inf, inf, inf}, {-inf, -inf, -inf}};
    uint32_t* nd = w.data() + 32 * (size_t)n;
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t ref = nd[24 + i], cnt = nd[28 + i];
        FBox b{{inf, inf, inf}, {-inf, -inf, -inf}};
        if (cnt) {
            for (uint32_t t = 0; t < cnt; ++t)
                for (int j = 0; j < 3; ++j)
                    for (int k = 0; k < 3; ++k) {
                        const float v = bitsf(w[32 * (size_t)nn + 12 * (size_t)(ref + t) + 4 * j + k]);
                        b.lo[k] = std::min(b.lo[k], v);
                        b.hi[k] = std::max(b.hi[k], v);
                    }
        } else if (ref != 0xffffffffu) {
            b = restate(w, nn, ref);
        } else {
            continue;
        }
        for (int k = 0; k < 3; ++k) {
            nd[8 * k + i] = fbits(std::nextafter(std::nextafter(b.lo[k], -inf), -inf));
            nd[8 * k + 4 + i] = fbits(std::nextafter(std::nextafter(b.hi[k], inf), inf));
            all.lo[k] = std::min(all.lo[k], b.lo[k]);
            all.hi[k] = std::max(all.hi[k], b.hi[k]);
        }
    }
    return all;
}

void check_steps() {
    const float inf = std::numeric_limits<float>::infinity();
    const uint32_t edge[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00000002u, 0x80000002u, 0x007fffffu,
                             0x807fffffu, 0x00800000u, 0x80800000u, 0x3f800000u, 0xbf800000u, 0x7f7fffffu, 0xff7fffffu,
                             0x7f7ffffeu, 0xff7ffffeu, 0x7f800000u, 0xff800000u, 0x34000000u, 0xb4000000u};
    for (uint32_t e : edge) {
        const float v = bitsf(e);
        expect(refit_next_down(e) == fbits(std::nextafter(v, -inf)), "next_down");
        expect(refit_next_up(e) == fbits(std::nextafter(v, inf)), "next_up");
        expect(refit_pad_lo(e) == fbits(std::nextafter(std::nextafter(v, -inf), -inf)), "pad_lo");
        expect(refit_pad_hi(e) == fbits(std::nextafter(std::nextafter(v, inf), inf)), "pad_hi");
        expect(refit_unkey(refit_key(e)) == e, "key round trip");
    }
    std::mt19937 rng(3);
    for (int i = 0; i < 200000; ++i) {
        const uint32_t a = rng(), b = rng();
        const float fa = bitsf(a), fb = bitsf(b);
        if (fa != fa || fb != fb) continue;
        expect(refit_next_down(a) == fbits(std::nextafter(fa, -inf)) && refit_next_up(a) == fbits(std::nextafter(fa, inf)),
               "random step");
        if (fa < fb) expect(refit_key(a) < refit_key(b), "key order");
        if (fa > fb) expect(refit_key(a) > refit_key(b), "key order");
    }
}

void check_scene(uint32_t nt, float spread, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    std::vector<float> pos;
    std::vector<uint32_t> ind;
    for (uint32_t t = 0; t < nt; ++t) {
        const float c[3] = {spread * U(rng), spread * U(rng), spread * U(rng)};
        for (int j = 0; j < 3; ++j) {
            for (int k = 0; k < 3; ++k) pos.push_back(c[k] + 0.3f * U(rng));
            ind.push_back(3 * t + j);
        }
    }
    if (nt > 4) {  // shared and repeated vertices
        ind[3] = ind[0];
        ind[7] = ind[2];
    }
    const uint32_t nv = (uint32_t)(pos.size() / 3);
    const FlatBvh b = build_bvh(pos.data(), nv, ind.data(), nt, nullptr, 2);
    const uint32_t nn = (uint32_t)(b.nodes.size() / 32);
    const std::vector<uint32_t> built = flatten(b);

    std::vector<uint32_t> parent(nn), inner(nn);
    expect(refit_topology(built.data(), nn, nt, parent.data(), inner.data()), "topology");
    uint32_t edges = 0;
    for (uint32_t n = 0; n < nn; ++n) {
        edges += inner[n];
        if (n) expect((parent[n] >> 2) < n && built[32 * (size_t)(parent[n] >> 2) + 24 + (parent[n] & 3u)] == n, "parent");
    }
    expect(nn == 0 || (edges == nn - 1 && parent[0] == kRefitNoParent), "tree edges");

    std::vector<uint32_t> w = built;
    refit_host(w.data(), nn, ind.data(), nt, pos.data());
    expect(w == built, "identity");

    for (int motion = 0; motion < 3; ++motion) {
        std::vector<float> p1 = pos;
        for (size_t i = 0; i < p1.size(); ++i) {
            if (motion == 0) p1[i] += 0.05f * U(rng);
            if (motion == 1 && i < p1.size() / 4) p1[i] += 5000.0f;
            if (motion == 2) p1[i] = (float)((double)p1[i] * 1e-41);
        }
        std::vector<uint32_t> got = built;
        refit_host(got.data(), nn, ind.data(), nt, p1.data());
        std::vector<uint32_t> want = built;
        for (uint32_t r = 0; r < nt; ++r) {
            const uint32_t prim = want[32 * (size_t)nn + 12 * (size_t)r + 3];
            for (int j = 0; j < 3; ++j)
                std::memcpy(&want[32 * (size_t)nn + 12 * (size_t)r + 4 * j], &p1[3 * (size_t)ind[3 * (size_t)prim + j]], 12);
        }
        if (nt) restate(want, nn, 0);
        expect(got == want, "moved");
        refit_host(got.data(), nn, ind.data(), nt, pos.data());
        expect(got == built, "return trip");
    }
}

void check_split_tree() {
    // long diagonal slivers: the spatial-split builder duplicates references
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    std::vector<float> pos;
    std::vector<uint32_t> ind;
    const uint32_t nt = 4000;
    for (uint32_t t = 0; t < nt; ++t) {
        const float c[3] = {10.0f * U(rng), 10.0f * U(rng), 10.0f * U(rng)};
        const float d[3] = {6.0f * U(rng), 6.0f * U(rng), 6.0f * U(rng)};
        for (int j = 0; j < 3; ++j) {
            for (int k = 0; k < 3; ++k) pos.push_back(c[k] + (j == 1 ? d[k] : 0.0f) + (j == 2 ? 0.05f * U(rng) : 0.0f));
            ind.push_back(3 * t + j);
        }
    }
    BvhOptions opt;
    opt.split_budget = 0.5;
    const FlatBvh b = build_bvh(pos.data(), 3 * nt, ind.data(), nt, nullptr, 2, opt);
    std::printf("split tree: spatial_splits %u references %u triangles %u\n", b.stats.spatial_splits, b.stats.references,
                nt);
    expect(b.stats.spatial_splits > 0 && b.tris.size() / 12 > nt, "the split tree has more records than triangles");
    const FlatBvh plain = build_bvh(pos.data(), 3 * nt, ind.data(), nt, nullptr, 2);
    expect(plain.stats.spatial_splits == 0 && plain.tris.size() / 12 == nt, "the default tree has none");
}
}  // namespace

int main() {
    check_steps();
    check_scene(0, 1.0f, 1);
    check_scene(1, 1.0f, 2);
    check_scene(5, 1.0f, 3);
    check_scene(300, 4.0f, 4);
    check_scene(6000, 20.0f, 5);
    check_split_tree();
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
