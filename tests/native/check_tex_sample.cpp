// check_tex_sample.cpp -- csrc/tex_sample.h on the host: librsd's sampler rule evaluated over a fixed case list and
// printed, inputs included, as integers and float bit patterns.  tests/test_tex_sample.py builds this with
// AddressSanitizer and UBSan (float-cast-overflow among its checks), recomputes every line with a float32 numpy
// restatement of its own and compares exactly.
//
// Lines (every float as the hex of its bits):
//   S W H kx fx ky fy u v | ix iy qx qy wx wy | wrap t00 t10 t01 t11 | clamp t00 t10 t01 t11 | lerp
//   A i n wrap | r            tex_addr
//   P uv n | r                tex_point
//   G W H g | minX minY maxX maxY
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "tex_sample.h"

using namespace rsd;

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// One coordinate of a case on an axis of n texels: the sample lies `frac` texels right of the centre of texel k
// (kinds 0-3), or is u = 0 / u = 1 exactly (kinds 4, 5: k is what the split must give)
struct Coord {
    int k, kind;
    float u;
};
static const float kFrac[4] = {0.0f, 77.3f / 256.0f, 255.4f / 256.0f, 255.9f / 256.0f};  // centre, mid, last below the carry, the carry

static std::vector<Coord> coords(int n) {
    std::vector<Coord> c;
    const int bases[] = {-n - 2, -n - 1, -2, -1, 0, n - 2, n - 1, n, n + 1};  // left of texel 0 ... right of texel n - 1
    for (int k : bases)
        for (int kind = 0; kind < 4; ++kind) c.push_back({k, kind, ((float)k + 0.5f + kFrac[kind]) / (float)n});
    for (int k = 1; k < n - 2; ++k) c.push_back({k, 0, ((float)k + 0.5f) / (float)n});  // the remaining pixel centres
    c.push_back({-1, 4, 0.0f});
    c.push_back({n - 1, 5, 1.0f});
    return c;
}

int main() {
    const int sizes[] = {1, 2, 3, 5};
    const float t00 = 0.125f, t10 = 0.7f, t01 = 1.0f / 3.0f, t11 = 0.9f;  // the four texels of the lerp
    for (int W : sizes)
        for (int H : sizes) {
            const std::vector<Coord> cx = coords(W), cy = coords(H);
            for (const Coord& x : cx)
                for (const Coord& y : cy) {
                    const TexSplit s = tex_split(W, H, x.u, y.u);
                    const TexTaps w = tex_taps(s, W, H, true), c = tex_taps(s, W, H, false);
                    std::printf("S %d %d %d %d %d %d %08x %08x | %d %d %08x %08x %08x %08x | %zu %zu %zu %zu | %zu %zu %zu %zu | %08x\n",
                                W, H, x.k, x.kind, y.k, y.kind, bits(x.u), bits(y.u), s.ix, s.iy, bits(s.qx), bits(s.qy),
                                bits(s.wx), bits(s.wy), w.t00, w.t10, w.t01, w.t11, c.t00, c.t10, c.t01, c.t11,
                                bits(tex_lerp(s, t00, t10, t01, t11)));
                }
        }
    for (int n : sizes)
        for (int i = -2 * n - 1; i <= 2 * n + 1; ++i)
            for (int wrap = 0; wrap < 2; ++wrap) std::printf("A %d %d %d | %d\n", i, n, wrap, tex_addr(i, n, wrap != 0));
    const float inf = std::numeric_limits<float>::infinity();
    const float uvs[] = {0.0f, -0.0f, 0.5f, std::nextafterf(1.0f, 0.0f), 1.0f, -0.25f, -1e-30f, 2.0f, 3e9f, -3e9f, 1e30f,
                         -1e30f, inf, -inf, std::numeric_limits<float>::quiet_NaN()};
    for (int n : sizes)
        for (float uv : uvs) std::printf("P %08x %d | %d\n", bits(uv), n, tex_point(uv, n));
    const uint32_t frames[][3] = {{1, 1, 0}, {5, 3, 1}, {97, 61, 16}, {1920, 1080, 64}, {1953, 1113, 0}};
    for (const auto& f : frames) {
        const GuardUv g = guard_uv(f[0], f[1], f[2]);
        std::printf("G %u %u %u | %08x %08x %08x %08x\n", f[0], f[1], f[2], bits(g.minX), bits(g.minY), bits(g.maxX), bits(g.maxY));
    }
    return 0;
}
