// check_sd_plan.cpp -- prints the SD trace's launch plan (csrc/sd_plan.h) of one call as "key value" lines, for
// tests/test_sd_plan.py.  Built from this file and csrc/sd_plan.cpp alone: that it links shows the plan is host only.
//
//   check_sd_plan [name=value ...]      the call (defaults below); the knobs come from the environment
//
// The camera looks straight down -Z from the origin: U = (aspect t, 0, 0), V = (0, t, 0), W = (0, 0, -1) with
// t = frameHeight / (2 focalLength) = 12 / 21 and aspect = w / h; nearZ 0.1, farZ 1000, no jitter.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "sd_plan.h"

int main(int argc, char** argv) {
    std::map<std::string, long> v = {
        {"w", 768}, {"h", 558}, {"zw", 0}, {"zh", 0}, {"start", 0}, {"step", 1}, {"n", -1},
        {"N", 4}, {"impl", RSD_SD_DEFAULT}, {"max_count", 8}, {"hit_order", RSD_HIT_ORDER_CANONICAL},
        {"ray_interval", 1}, {"guard", 0}, {"use16", 0}, {"normalize", 0}, {"alpha_test", 0}, {"flags", 0},
        {"raymin", 1}, {"raymax", 1}, {"counters", 0}, {"cu", 256}, {"depth", 12}, {"entry", 1}, {"primrec", 1},
        {"alphadata", 0}, {"tris", 1000}, {"nullarg", 0}};
    for (int i = 1; i < argc; ++i) {
        const char* eq = std::strchr(argv[i], '=');
        const std::string name(argv[i], eq ? (size_t)(eq - argv[i]) : std::strlen(argv[i]));
        if (!eq || !v.count(name)) {
            std::fprintf(stderr, "check_sd_plan: unknown argument '%s'\n", argv[i]);
            return 2;
        }
        v[name] = std::atol(eq + 1);
    }
    rsd::SdPlanIn in;
    in.nullArg = v["nullarg"] != 0;
    in.sdW = (uint32_t)v["w"];
    in.sdH = (uint32_t)v["h"];
    in.zW = v["zw"] ? (uint32_t)v["zw"] : in.sdW;  // the depth buffer: the map's size unless given
    in.zH = v["zh"] ? (uint32_t)v["zh"] : in.sdH;
    in.start = (uint32_t)v["start"];
    in.step = (uint32_t)v["step"];
    in.n = v["n"] >= 0 ? (uint32_t)v["n"] : (in.sdH + rsd::kTile - 1) / rsd::kTile;  // every tile row unless given
    in.params.sample_count = (uint32_t)v["N"];
    in.params.implementation = (uint32_t)v["impl"];
    in.params.max_count = (uint32_t)v["max_count"];
    in.params.guard_band = (int32_t)v["guard"];
    in.params.ray_interval = (uint32_t)v["ray_interval"];
    in.params.hit_order = (uint32_t)v["hit_order"];
    in.params.use_16bit = (uint32_t)v["use16"];
    in.params.normalize = (uint32_t)v["normalize"];
    in.params.alpha_test = (uint32_t)v["alpha_test"];
    in.flags = (uint32_t)v["flags"];
    in.rayMin = v["raymin"] != 0;
    in.rayMax = v["raymax"] != 0;
    in.counters = v["counters"] != 0;
    in.cuCount = (int)v["cu"];
    in.wideDepth = (uint32_t)v["depth"];
    in.entryTable = v["entry"] != 0;
    in.primRec = v["primrec"] != 0;
    in.alphaData = v["alphadata"] != 0;
    in.triangleCount = (uint32_t)v["tris"];
    const float t = 12.0f / 21.0f, aspect = in.sdH ? (float)in.sdW / (float)in.sdH : 1.0f;
    in.cam.U[0] = aspect * t;
    in.cam.V[1] = t;
    in.cam.W[2] = -1.0f;
    in.cam.nearZ = 0.1f;
    in.cam.farZ = 1000.0f;
    in.cam.focalLength = 21.0f;
    in.cam.frameHeight = 24.0f;
    in.cam.aspectRatio = aspect;

    rsd::SdPlan p, again;
    std::string err, err2;
    const rsd::SdKnobs knobs = rsd::sd_knobs_from_env();
    const rsd_status st = rsd::sd_plan(in, knobs, &p, &err);
    const rsd_status st2 = rsd::sd_plan(in, knobs, &again, &err2);  // equal inputs: an equal plan
    std::printf("status %d\n", (int)st);
    std::printf("error %s\n", err.c_str());
    std::printf("repeatable %d\n", st == st2 && err == err2 && p.walk == again.walk && p.workspaceBytes == again.workspaceBytes &&
                                       p.persistentBlocks == again.persistentBlocks && p.cosLower == again.cosLower);
    if (st != RSD_OK) return 0;
#define U(f) std::printf(#f " %llu\n", (unsigned long long)p.f)
#define I(f) std::printf(#f " %lld\n", (long long)p.f)
#define F(f) std::printf(#f " %.17g\n", (double)p.f)
    U(empty); U(launch); U(buildKey); I(walk); I(walkReported); U(K); U(ROW); U(split); U(spec); U(counters);
    I(pool); I(poolSoft); U(quadStack); U(ldsBytes);
    std::printf("setupGrid %u %u\nclassGrid %u %u\n", p.setupGrid[0], p.setupGrid[1], p.classGrid[0], p.classGrid[1]);
    U(liveBlocks); U(rasterBlocks); U(persistentBlocks); U(hybridRowBlocks); U(rowPrio); U(prio);
    U(lpt); F(lptLen); U(spread); U(qrange); U(diag); U(entOn); U(deadFast); F(cosLower);
    U(twoPass); U(touchCap); U(partCap); U(tileSig); U(tileCount);
    U(queueBytes); U(keysOff); U(keyBytes); U(entOff); U(entBytes); U(touchOff); U(touchBytes); U(workspaceBytes);
    U(rayLogBytes);
    U(keys64Bytes); U(slotOff); U(slotBytes); U(tileRecOff); U(tileRecBytes); U(liveTilesOff); U(liveTilesBytes);
    U(rasterBytes);
    std::printf("projU %.9g %.9g %.9g\nprojV %.9g %.9g %.9g\nprojW %.9g %.9g %.9g\ncamWn %.9g %.9g %.9g\n", p.projU[0],
                p.projU[1], p.projU[2], p.projV[0], p.projV[1], p.projV[2], p.projW[0], p.projW[1], p.projW[2],
                p.camWn[0], p.camWn[1], p.camWn[2]);
    F(wClip); I(tilesW); U(rayTabBytes);
    std::printf("kQueueParts %u\nkBlock %d\nkEntryCap %u\nkPlanBuildKey %u\n", rsd::kQueueParts, rsd::kBlock,
                rsd::kEntryCap, rsd::kPlanBuildKey);
    return 0;
}
