// check_npy.cpp -- a stand-alone driver of csrc/host/npy.h for tests/test_convnet.py, built with
// -fsanitize=address,undefined and run as its own process: for every file named on the command line it prints one line,
// "ok <dims> <shape...> <sum of the values>" or "error <message>".  The parser is header-only host code, so the
// sanitizers see all of it.
#include <cstdio>

#include "host/npy.h"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        rsd::npy::Array a;
        std::string err;
        if (!rsd::npy::load(argv[i], a, err)) {
            std::printf("error %s\n", err.c_str());
            continue;
        }
        double sum = 0.0;
        for (float v : a.data) sum += v;
        std::printf("ok %zu", a.shape.size());
        for (auto d : a.shape) std::printf(" %llu", (unsigned long long)d);
        std::printf(" %.9g\n", sum);
    }
    return 0;
}
