/*
 * depth_peel_ref.c -- CPU statement of the DepthPeeling semantics (include/rsd.h rsd_depth_peel),
 * the checker of tests/test_depth_peel.py and tests/test_gpu_depth_peel.py.
 *
 * TEST INFRASTRUCTURE ONLY; it shares no code with librsd.  A brute-force loop over ALL triangles
 * per pixel (no BVH, no lower bound), threaded over rows:
 *   ray     pixel-centre pinhole ray, d = normalize(dir((x+.5)/W - jitterX, (y+.5)/H + jitterY)),
 *           cosT = dot(normalize(W), d), interval [nearZ / cosT, farZ / cosT];
 *   hit     the oracle's watertight test (ocpu_intersect), culling, alpha test at LOD 0
 *           (ocpu_alpha_fails) for triangles whose flags carry bit 2;
 *   peel    a hit of zlin = t * cosT is discarded iff zlin <= prev + minSeparation;
 *   result  the surviving hit with the smallest (t, prim): zlin (cleared: farZ) when linear_out,
 *           else farZ (zlin - nearZ) / (zlin (farZ - nearZ)) (cleared: 1).
 * tests/test_depth_peel.py pins it to the oracle's G-buffers at prev = 0, minSeparation = 0.
 *
 * Built by the tests with gcc -O2 -ffp-contract=off -pthread against the oracle's shared library.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

#include "rsd_oracle.h"

typedef struct {
    const oscene* s;
    int has_alpha;
    const float* pos;
    const uint32_t* idx;
    const uint32_t* flags;
    uint32_t nt;
    const ocam* c;
    uint32_t W, H, cull;
    const float* prev;
    float minSep;
    uint32_t linear_out;
    float* out;
    uint32_t y0, y1;
} job_t;

static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void normalize3(const float v[3], float r[3])
{
    float inv = 1.0f / sqrtf(dot3(v, v));
    r[0] = v[0] * inv; r[1] = v[1] * inv; r[2] = v[2] * inv;
}

/* Camera.slang:73-90 computeNonNormalizedRayDirPinhole */
static void ray_dir(const ocam* c, float px, float py, float out[3])
{
    float ndcx = 2.0f * px + -1.0f;
    float ndcy = -2.0f * py + 1.0f;
    for (int i = 0; i < 3; ++i) out[i] = ndcx * c->U[i] + ndcy * c->V[i] + c->W[i];
}

/* det > 0: counter-clockwise from the ray origin = front face unless frontFaceCW (bit 1);
 * double-sided (bit 0) is never culled.  cull: 0 none, 1 back, 2 front */
static int is_culled(float det, uint32_t flags, uint32_t cull)
{
    if (cull == 0 || (flags & 1u)) return 0;
    int front = (det > 0.0f) != ((flags & 2u) != 0);
    return cull == 1 ? !front : front;
}

static void* rows(void* arg)
{
    const job_t* j = (const job_t*)arg;
    const ocam* c = j->c;
    float wn[3];
    normalize3(c->W, wn);
    for (uint32_t y = j->y0; y < j->y1; ++y)
        for (uint32_t x = 0; x < j->W; ++x) {
            float px = ((float)x + 0.5f) / (float)j->W + -c->jitterX;
            float py = ((float)y + 0.5f) / (float)j->H + c->jitterY;
            float dn[3], d[3];
            ray_dir(c, px, py, dn);
            normalize3(dn, d);
            const float cosT = dot3(wn, d);
            const float invCos = 1.0f / cosT;
            const float tmin = c->nearZ * invCos, tmax = c->farZ * invCos;
            const size_t o = (size_t)y * j->W + x;
            const float thr = j->prev[o] + j->minSep;
            int found = 0;
            float bestT = INFINITY;
            uint32_t bestP = 0xffffffffu;
            for (uint32_t prim = 0; prim < j->nt; ++prim) {
                const float* v0 = j->pos + 3 * (size_t)j->idx[3 * prim];
                const float* v1 = j->pos + 3 * (size_t)j->idx[3 * prim + 1];
                const float* v2 = j->pos + 3 * (size_t)j->idx[3 * prim + 2];
                float t, bu, bv, det;
                if (!ocpu_intersect(c->posW, d, v0, v1, v2, &t, &bu, &bv, &det)) continue;
                if (!(t >= tmin && t <= tmax)) continue;
                if (is_culled(det, j->flags[prim], j->cull)) continue;
                const float zlin = t * cosT;
                if (zlin <= thr) continue; /* DepthPeeling.3d.slang: discard */
                if (found && !(t < bestT || (t == bestT && prim < bestP))) continue;
                if (j->has_alpha && (j->flags[prim] & 4u) && ocpu_alpha_fails(j->s, prim, bu, bv, 0, t, d, 0.0f))
                    continue;
                found = 1;
                bestT = t;
                bestP = prim;
            }
            if (!found) {
                j->out[o] = j->linear_out ? c->farZ : 1.0f;
            } else {
                const float zlin = bestT * cosT;
                j->out[o] = j->linear_out ? zlin : c->farZ * (zlin - c->nearZ) / (zlin * (c->farZ - c->nearZ));
            }
        }
    return NULL;
}

/* s: the oracle scene of the same geometry (read by ocpu_alpha_fails only); has_alpha: it holds
 * alpha materials.  positions float3[], indices uint32[3 nt], flags uint32[nt]. */
void depth_peel_ref(const oscene* s, int has_alpha, const float* positions, const uint32_t* indices,
                    const uint32_t* flags, uint32_t nt, const ocam* cam, uint32_t W, uint32_t H, uint32_t cull,
                    const float* prev, float min_separation, uint32_t linear_out, float* out, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if ((uint32_t)nthreads > H) nthreads = (int)H;
    job_t jobs[64];
    pthread_t th[64];
    for (int i = 0; i < nthreads; ++i) {
        job_t j = {s, has_alpha, positions, indices, flags, nt, cam, W, H, cull, prev, min_separation, linear_out,
                   out, (uint32_t)((uint64_t)H * i / nthreads), (uint32_t)((uint64_t)H * (i + 1) / nthreads)};
        jobs[i] = j;
        pthread_create(&th[i], NULL, rows, &jobs[i]);
    }
    for (int i = 0; i < nthreads; ++i) pthread_join(th[i], NULL);
}
