/*
 * mvec_ref.c -- CPU statement of the motion vectors of moving geometry (include/rsd.h rsd_gbuffer_motion),
 * the checker of tests/test_mvec.py, tests/test_gpu_mvec.py and tests/test_gpu_graph_mvec.py.
 *
 * TEST INFRASTRUCTURE ONLY; it shares no code with librsd.  A brute-force loop over ALL triangles per pixel
 * (no BVH), threaded over rows:
 *   ray     pixel-centre pinhole ray, d = normalize(dir((x+.5)/W - jitterX, (y+.5)/H + jitterY)),
 *           cosT = dot(normalize(W), d), interval [nearZ / cosT, farZ / cosT];
 *   hit     the oracle's watertight test (ocpu_intersect) on the CURRENT positions, culling, alpha test at
 *           LOD 0 (ocpu_alpha_fails) for triangles whose flags carry bit 2; the winner is the smallest (t, prim);
 *   motion  for the winner with vertices v0, v1, v2 (current) and barycentrics bu (weighs v1), bv (weighs v2):
 *             d_j = prev_positions[i_j] - v_j          b0 = (1 - bu) - bv
 *             D = (b0 d0 + bu d1) + bv d2              P = o + d t          P_prev = P + D
 *             rel = P_prev - prev.posW;  pa, pb, pw = dot(rel, U/|U|^2), dot(rel, V/|V|^2), dot(rel, W/|W|^2)
 *             of the previous camera (the three vectors in double, rounded once; a dot is (x + y) + z)
 *             mvec = ((pa / pw + 1) 0.5 - u, (1 - pb / pw) 0.5 - v) when pw > 0, else (2, 2)
 *             mvecW = (D, 0)
 *           with u = (x + .5) / W, v = (y + .5) / H; every product and sum rounded to float32 on its own;
 *   miss    mvec = (0, 0), mvecW = 0, prim = 0xffffffff.
 * It also reports the winner itself (prim; t, bu, bv), from which tests/mvec_checker.py evaluates the same
 * formula in float64.
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
    const float* prev;
    const uint32_t* idx;
    const uint32_t* flags;
    uint32_t nt;
    const ocam* c;
    const ocam* pc;
    uint32_t W, H, cull;
    float* mvec;
    float* mvecW;
    uint32_t* prim;
    float* tuv;
    float pU[3], pV[3], pW[3];
    uint32_t y0, y1;
} job_t;

static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void normalize3(const float v[3], float r[3])
{
    float inv = 1.0f / sqrtf(dot3(v, v));
    r[0] = v[0] * inv; r[1] = v[1] * inv; r[2] = v[2] * inv;
}

static void ray_dir(const ocam* c, float px, float py, float out[3])
{
    float ndcx = 2.0f * px + -1.0f;
    float ndcy = -2.0f * py + 1.0f;
    for (int i = 0; i < 3; ++i) out[i] = ndcx * c->U[i] + ndcy * c->V[i] + c->W[i];
}

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
            const float u = ((float)x + 0.5f) / (float)j->W, v = ((float)y + 0.5f) / (float)j->H;
            float dn[3], d[3];
            ray_dir(c, u + -c->jitterX, v + c->jitterY, dn);
            normalize3(dn, d);
            const float cosT = dot3(wn, d);
            const float invCos = 1.0f / cosT;
            const float tmin = c->nearZ * invCos, tmax = c->farZ * invCos;
            const size_t o = (size_t)y * j->W + x;
            int found = 0;
            float bestT = INFINITY, bestU = 0.0f, bestV = 0.0f;
            uint32_t bestP = 0xffffffffu;
            for (uint32_t prim = 0; prim < j->nt; ++prim) {
                const float* v0 = j->pos + 3 * (size_t)j->idx[3 * prim];
                const float* v1 = j->pos + 3 * (size_t)j->idx[3 * prim + 1];
                const float* v2 = j->pos + 3 * (size_t)j->idx[3 * prim + 2];
                float t, bu, bv, det;
                if (!ocpu_intersect(c->posW, d, v0, v1, v2, &t, &bu, &bv, &det)) continue;
                if (!(t >= tmin && t <= tmax)) continue;
                if (is_culled(det, j->flags[prim], j->cull)) continue;
                if (found && !(t < bestT || (t == bestT && prim < bestP))) continue;
                if (j->has_alpha && (j->flags[prim] & 4u) && ocpu_alpha_fails(j->s, prim, bu, bv, 0, t, d, 0.0f))
                    continue;
                found = 1;
                bestT = t;
                bestU = bu;
                bestV = bv;
                bestP = prim;
            }
            j->prim[o] = bestP;
            j->tuv[3 * o] = found ? bestT : 0.0f;
            j->tuv[3 * o + 1] = bestU;
            j->tuv[3 * o + 2] = bestV;
            for (int k = 0; k < 4; ++k) j->mvecW[4 * o + k] = 0.0f;
            j->mvec[2 * o] = 0.0f;
            j->mvec[2 * o + 1] = 0.0f;
            if (!found) continue;
            float D[3], rel[3];
            const float b0 = (1.0f - bestU) - bestV;
            for (int k = 0; k < 3; ++k) {
                const uint32_t i0 = j->idx[3 * bestP], i1 = j->idx[3 * bestP + 1], i2 = j->idx[3 * bestP + 2];
                const float d0 = j->prev[3 * (size_t)i0 + k] - j->pos[3 * (size_t)i0 + k];
                const float d1 = j->prev[3 * (size_t)i1 + k] - j->pos[3 * (size_t)i1 + k];
                const float d2 = j->prev[3 * (size_t)i2 + k] - j->pos[3 * (size_t)i2 + k];
                D[k] = (b0 * d0 + bestU * d1) + bestV * d2;
                const float P = c->posW[k] + d[k] * bestT;
                rel[k] = (P + D[k]) - j->pc->posW[k];
                j->mvecW[4 * o + k] = D[k];
            }
            const float pa = rel[0] * j->pU[0] + rel[1] * j->pU[1] + rel[2] * j->pU[2];
            const float pb = rel[0] * j->pV[0] + rel[1] * j->pV[1] + rel[2] * j->pV[2];
            const float pw = rel[0] * j->pW[0] + rel[1] * j->pW[1] + rel[2] * j->pW[2];
            if (pw > 0.0f) {
                j->mvec[2 * o] = (pa / pw + 1.0f) * 0.5f - u;
                j->mvec[2 * o + 1] = (1.0f - pb / pw) * 0.5f - v;
            } else {
                j->mvec[2 * o] = 2.0f;
                j->mvec[2 * o + 1] = 2.0f;
            }
        }
    return NULL;
}

static double ddot(const float a[3], const float b[3])
{
    return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2];
}

/* s: the oracle scene of the CURRENT geometry (read by ocpu_alpha_fails only); has_alpha: it holds alpha
 * materials.  positions / prev_positions float3[], indices uint32[3 nt], flags uint32[nt].
 * mvec float[H][W][2], mvecW float[H][W][4], prim uint32[H][W], tuv float[H][W][3] = (t, bu, bv). */
void mvec_ref(const oscene* s, int has_alpha, const float* positions, const float* prev_positions,
              const uint32_t* indices, const uint32_t* flags, uint32_t nt, const ocam* cam, const ocam* prev_cam,
              uint32_t W, uint32_t H, uint32_t cull, float* mvec, float* mvecW, uint32_t* prim, float* tuv,
              int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if ((uint32_t)nthreads > H) nthreads = (int)H;
    job_t jobs[64];
    pthread_t th[64];
    const double uu = ddot(prev_cam->U, prev_cam->U), vv = ddot(prev_cam->V, prev_cam->V),
                 ww = ddot(prev_cam->W, prev_cam->W);
    for (int i = 0; i < nthreads; ++i) {
        job_t j = {s, has_alpha, positions, prev_positions, indices, flags, nt, cam, prev_cam, W, H, cull, mvec, mvecW,
                   prim, tuv, {0}, {0}, {0}, (uint32_t)((uint64_t)H * i / nthreads),
                   (uint32_t)((uint64_t)H * (i + 1) / nthreads)};
        for (int k = 0; k < 3; ++k) {
            j.pU[k] = (float)(prev_cam->U[k] / uu);
            j.pV[k] = (float)(prev_cam->V[k] / vv);
            j.pW[k] = (float)(prev_cam->W[k] / ww);
        }
        jobs[i] = j;
        pthread_create(&th[i], NULL, rows, &jobs[i]);
    }
    for (int i = 0; i < nthreads; ++i) pthread_join(th[i], NULL);
}
