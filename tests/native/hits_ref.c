/*
 * hits_ref.c -- brute-force any-hit reference of the SD rays, and a CPU model of the per-lane stack
 * of librsd's depth-first walks.  The checker of tests/test_adversarial_walk.py and
 * tests/test_gpu_adversarial_walk.py.
 *
 * TEST INFRASTRUCTURE ONLY; it shares no code with librsd.
 *
 * hits_ref: per SD texel the ray of ocpu_sd_ray, a loop over ALL triangles (no BVH, no bound) with
 *   the oracle's watertight test (ocpu_intersect), hits with TMin <= t <= TMax kept, culling applied,
 *   the alpha test at LOD 0 (ocpu_alpha_fails) for triangles whose flags carry bit 2.  Per texel: the
 *   number of hits and the first `cap` of them in ascending (t, prim) order as t, prim and t * cosT
 *   (slots beyond the count: t = +inf, prim = 0xffffffff, t * cosT = +inf).
 *
 * stack_model: librsd's one per-lane walk, the nearest-first depth-first walk_lane with its LaneStack
 *   (csrc/bvh_traverse.h), restated over librsd's exported BVH as the G-buffer kernel calls it: the primary ray of
 *   every pixel, the upper bound min(TMax, closest t), no lower bound beyond TMin.  Per pixel the high-water mark
 *   of the stack, and the closest key (t, prim) the walk ends with.  A mark above 16 means the walk left the LDS
 *   stack for the private spill arrays.  The depth peel (csrc/depth_peel.hip) calls the same walk on the same rays
 *   with a lower bound raised by prev, which prunes children and clamps their sort and stack keys: it is the
 *   modelled walk only when prev + separation <= 0.  The AO rays (csrc/svao_rt.hip, a written-out copy of the
 *   loop) walk secondary rays, which the model does not cover.
 *
 * Built by the tests with gcc -O2 -ffp-contract=off -pthread against the oracle's shared library.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "rsd_oracle.h"

static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void normalize3(const float v[3], float r[3])
{
    float inv = 1.0f / sqrtf(dot3(v, v));
    r[0] = v[0] * inv; r[1] = v[1] * inv; r[2] = v[2] * inv;
}
static uint32_t asuint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* det > 0: counter-clockwise from the ray origin = front face unless frontFaceCW (bit 1);
 * double-sided (bit 0) is never culled.  cull: 0 none, 1 back, 2 front */
static int is_culled(float det, uint32_t flags, uint32_t cull)
{
    if (cull == 0 || (flags & 1u)) return 0;
    int front = (det > 0.0f) != ((flags & 2u) != 0);
    return cull == 1 ? !front : front;
}

static int key_before(float ta, uint32_t pa, float tb, uint32_t pb) { return ta < tb || (ta == tb && pa < pb); }

typedef struct { float t; uint32_t prim; } hkey;

static int key_cmp(const void* a, const void* b)
{
    const hkey* x = (const hkey*)a;
    const hkey* y = (const hkey*)b;
    if (key_before(x->t, x->prim, y->t, y->prim)) return -1;
    if (key_before(y->t, y->prim, x->t, x->prim)) return 1;
    return 0;
}

/* ------------------------------------------------------------------ brute-force hit lists */
typedef struct {
    const oscene* s;
    int has_alpha;
    const float* pos;
    const uint32_t* idx;
    const uint32_t* flags;
    uint32_t nt;
    const ocam* c;
    const osd_params* p;
    const float* z;
    uint32_t zW, zH;
    const uint32_t *rmin, *rmax;
    uint32_t sdW, sdH, cap;
    uint32_t* count;
    float* t;
    uint32_t* prim;
    float* zt;
    uint32_t y0, y1;
} hits_job;

static void* hits_rows(void* arg)
{
    const hits_job* j = (const hits_job*)arg;
    hkey* all = (hkey*)malloc(sizeof(hkey) * (j->nt ? j->nt : 1u));
    for (uint32_t y = j->y0; y < j->y1; ++y)
        for (uint32_t x = 0; x < j->sdW; ++x) {
            float od[6], tmin, tmax, cosT;
            ocpu_sd_ray(j->c, j->p, j->z, j->zW, j->zH, j->rmin, j->rmax, j->sdW, j->sdH, x, y, od, &tmin, &tmax, &cosT);
            uint32_t n = 0;
            if (tmin <= tmax)
                for (uint32_t prim = 0; prim < j->nt; ++prim) {
                    const float* v0 = j->pos + 3 * (size_t)j->idx[3 * prim];
                    const float* v1 = j->pos + 3 * (size_t)j->idx[3 * prim + 1];
                    const float* v2 = j->pos + 3 * (size_t)j->idx[3 * prim + 2];
                    float t, bu, bv, det;
                    if (!ocpu_intersect(od, od + 3, v0, v1, v2, &t, &bu, &bv, &det)) continue;
                    if (!(t >= tmin && t <= tmax)) continue;
                    if (is_culled(det, j->flags[prim], j->p->cull_mode)) continue;
                    if (j->has_alpha && (j->flags[prim] & 4u) && ocpu_alpha_fails(j->s, prim, bu, bv, 0, t, od + 3, 0.0f))
                        continue;
                    all[n].t = t;
                    all[n].prim = prim;
                    ++n;
                }
            qsort(all, n, sizeof(hkey), key_cmp);
            const size_t o = (size_t)y * j->sdW + x;
            j->count[o] = n;
            for (uint32_t k = 0; k < j->cap; ++k) {
                j->t[o * j->cap + k] = k < n ? all[k].t : INFINITY;
                j->prim[o * j->cap + k] = k < n ? all[k].prim : 0xffffffffu;
                j->zt[o * j->cap + k] = k < n ? all[k].t * cosT : INFINITY;
            }
        }
    free(all);
    return NULL;
}

/* s: the oracle scene of the same geometry (read by ocpu_alpha_fails only); has_alpha: it holds alpha
 * materials.  positions float3[], indices uint32[3 nt], flags uint32[nt]; z, rmin, rmax, sdW, sdH as
 * ocpu_sd_trace takes them.  count uint32[sdH sdW]; t, prim, zt [sdH sdW cap]. */
void hits_ref(const oscene* s, int has_alpha, const float* positions, const uint32_t* indices, const uint32_t* flags,
              uint32_t nt, const ocam* cam, const osd_params* p, const float* z, uint32_t zW, uint32_t zH,
              const uint32_t* rmin, const uint32_t* rmax, uint32_t sdW, uint32_t sdH, uint32_t cap, uint32_t* count,
              float* t, uint32_t* prim, float* zt, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if ((uint32_t)nthreads > sdH) nthreads = (int)sdH;
    hits_job jobs[64];
    pthread_t th[64];
    for (int i = 0; i < nthreads; ++i) {
        hits_job j = {s, has_alpha, positions, indices, flags, nt, cam, p, z, zW, zH, rmin, rmax, sdW, sdH, cap,
                      count, t, prim, zt, (uint32_t)((uint64_t)sdH * i / nthreads),
                      (uint32_t)((uint64_t)sdH * (i + 1) / nthreads)};
        jobs[i] = j;
        pthread_create(&th[i], NULL, hits_rows, &jobs[i]);
    }
    for (int i = 0; i < nthreads; ++i) pthread_join(th[i], NULL);
}

/* ------------------------------------------------------------------ the per-lane stack, modelled */
#define MODEL_STACK 128 /* the model's own stack; the marks it reports are asserted far below this */

typedef struct { float invd[3], olo[3], ohi[3]; } box_ray;

static void box_setup(box_ray* b, const float o[3], const float d[3])
{
    for (int i = 0; i < 3; ++i) {
        const float v = fabsf(d[i]) > 1e-20f ? d[i] : copysignf(1e-20f, d[i]);
        b->invd[i] = 1.0f / v;
        /* a clamped axis (d = 0): the slab widened by e = 1e20 (2^-22 |o| + 1e-10), the lo plane's subtrahend moved
         * one way, the hi plane's the other, by the sign of 1 / d; every other axis: o / d itself */
        const float c = o[i] * b->invd[i];
        const int clamped = !(fabsf(d[i]) > 1e-20f);
        const float e = fabsf(b->invd[i]) * (fabsf(o[i]) * 2.384185791015625e-07f + 1e-10f);
        b->olo[i] = !clamped ? c : (b->invd[i] > 0.0f ? c + e : c - e);
        b->ohi[i] = !clamped ? c : (b->invd[i] > 0.0f ? c - e : c + e);
    }
}

/* the slab test of the walks: one fused multiply-add per plane, entry / exit widened by a relative 1e-5 */
static int box_test(const box_ray* b, const float* nb, int q, float tlo, float thi, float* tnear)
{
    const float x0 = fmaf(nb[q], b->invd[0], -b->olo[0]), x1 = fmaf(nb[4 + q], b->invd[0], -b->ohi[0]);
    const float y0 = fmaf(nb[8 + q], b->invd[1], -b->olo[1]), y1 = fmaf(nb[12 + q], b->invd[1], -b->ohi[1]);
    const float z0 = fmaf(nb[16 + q], b->invd[2], -b->olo[2]), z1 = fmaf(nb[20 + q], b->invd[2], -b->ohi[2]);
    float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    const float m = 1e-5f * (fabsf(tn) + fabsf(tf));
    tn -= m;
    tf += m;
    *tnear = tn;
    return fmaxf(tn, tlo) <= fminf(tf, thi);
}

static void swap_if_nearer(float* k, uint32_t* it, int a, int b)
{
    if (k[b] < k[a]) {
        const float t = k[a]; k[a] = k[b]; k[b] = t;
        const uint32_t u = it[a]; it[a] = it[b]; it[b] = u;
    }
}

typedef struct {
    const float* bvh;
    uint32_t triOff;
    const ocam* c;
    uint32_t W, H, cull;
    uint32_t* mark;
    float* bestT;
    uint32_t* bestP;
    uint32_t y0, y1;
} model_job;

static void* model_rows(void* arg)
{
    const model_job* j = (const model_job*)arg;
    const uint32_t LEAF = 0x80000000u, OFF = 0x1fffffffu, NONE = 0xffffffffu;
    const ocam* c = j->c;
    float wn[3];
    normalize3(c->W, wn);
    for (uint32_t y = j->y0; y < j->y1; ++y)
        for (uint32_t x = 0; x < j->W; ++x) {
            /* the pixel-centre pinhole ray of the G-buffer and the peel */
            const float px = ((float)x + 0.5f) / (float)j->W + -c->jitterX;
            const float py = ((float)y + 0.5f) / (float)j->H + c->jitterY;
            const float ndcx = 2.0f * px + -1.0f, ndcy = -2.0f * py + 1.0f;
            float dn[3], d[3];
            for (int i = 0; i < 3; ++i) dn[i] = ndcx * c->U[i] + ndcy * c->V[i] + c->W[i];
            normalize3(dn, d);
            const float invCos = 1.0f / dot3(wn, d);
            const float tmin = c->nearZ * invCos, tmax = c->farZ * invCos;
            box_ray b;
            box_setup(&b, c->posW, d);
            uint32_t stItem[MODEL_STACK];
            float stT[MODEL_STACK];
            int sp = 0, high = 0;
            float bestT = INFINITY;
            uint32_t bestP = NONE;
            uint32_t item = 0; /* root */
            for (;;) {
                const uint32_t off = item & OFF;
                uint32_t next = NONE;
                if (item & LEAF) {
                    const uint32_t n = ((item >> 29) & 3u) + 1u;
                    for (uint32_t q = 0; q < n; ++q) {
                        const float* tp = j->bvh + 4u * (off + 3u * q); /* {v0, prim}{v1, flags}{v2, 0} */
                        float t, bu, bv, det;
                        if (!ocpu_intersect(c->posW, d, tp, tp + 4, tp + 8, &t, &bu, &bv, &det)) continue;
                        if (!(t >= tmin && t <= tmax)) continue;
                        if (is_culled(det, asuint(tp[7]), j->cull)) continue;
                        if (!key_before(t, asuint(tp[3]), bestT, bestP)) continue;
                        bestT = t;
                        bestP = asuint(tp[3]);
                    }
                } else {
                    const float* nb = j->bvh + 4u * off;
                    const float thi = fminf(tmax, bestT);
                    float k[4];
                    uint32_t it[4];
                    for (int q = 0; q < 4; ++q) {
                        const uint32_t ref = asuint(nb[24 + q]), cnt = asuint(nb[28 + q]);
                        float tn = 0.0f;
                        const int hit = ref != NONE && box_test(&b, nb, q, tmin, thi, &tn);
                        k[q] = hit ? tn : INFINITY;
                        it[q] = hit ? (cnt ? (LEAF | ((cnt - 1u) << 29) | (j->triOff + 3u * ref)) : 8u * ref) : NONE;
                    }
                    swap_if_nearer(k, it, 0, 1); swap_if_nearer(k, it, 2, 3);
                    swap_if_nearer(k, it, 0, 2); swap_if_nearer(k, it, 1, 3);
                    swap_if_nearer(k, it, 1, 2);
                    for (int q = 3; q >= 1; --q) /* the nearest of the rest on top */
                        if (it[q] != NONE && sp < MODEL_STACK) {
                            stItem[sp] = it[q];
                            stT[sp] = k[q];
                            ++sp;
                        }
                    if (sp > high) high = sp;
                    next = it[0];
                }
                if (next == NONE) {
                    const float thi = fminf(tmax, bestT);
                    while (sp > 0) {
                        --sp;
                        if (stT[sp] <= thi) { next = stItem[sp]; break; }
                    }
                    if (next == NONE) break;
                }
                item = next;
            }
            const size_t o = (size_t)y * j->W + x;
            j->mark[o] = (uint32_t)high;
            j->bestT[o] = bestT;
            j->bestP[o] = bestP;
        }
    return NULL;
}

/* bvh: the rsd_scene_export_bvh / rsd_bvh_build bytes, tri_offset in float4 units.  mark, best_t, best_prim
 * [H W]: the stack's high-water mark, and the closest key the walk found (+inf, 0xffffffff: none). */
void stack_model(const float* bvh, uint32_t tri_offset, const ocam* cam, uint32_t W, uint32_t H, uint32_t cull,
                 uint32_t* mark, float* best_t, uint32_t* best_prim, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if ((uint32_t)nthreads > H) nthreads = (int)H;
    model_job jobs[64];
    pthread_t th[64];
    for (int i = 0; i < nthreads; ++i) {
        model_job j = {bvh, tri_offset, cam, W, H, cull, mark, best_t, best_prim,
                       (uint32_t)((uint64_t)H * i / nthreads), (uint32_t)((uint64_t)H * (i + 1) / nthreads)};
        jobs[i] = j;
        pthread_create(&th[i], NULL, model_rows, &jobs[i]);
    }
    for (int i = 0; i < nthreads; ++i) pthread_join(th[i], NULL);
}
