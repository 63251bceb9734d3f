// npy.h -- a small reader of NumPy .npy files for the host side of librsd (no HIP dependency): format 1.0 and 2.0,
// dtype '<f4', C order.  Everything else -- another dtype or byte order, Fortran order, a truncated header or payload,
// a shape whose product overflows or disagrees with the file size -- is an error with a message.  The header is the
// Python dict literal NumPy writes: {'descr': '<f4', 'fortran_order': False, 'shape': (3, 3, 4, 8), }.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace rsd::npy {

struct Array {
    std::vector<uint64_t> shape;
    std::vector<float> data;
};

namespace detail {
// the value text after 'key': in the header dict, or npos
inline size_t value_of(const std::string& h, const char* key) {
    const std::string k = std::string("'") + key + "'";
    size_t p = h.find(k);
    if (p == std::string::npos) return p;
    p = h.find(':', p + k.size());
    if (p == std::string::npos) return p;
    ++p;
    while (p < h.size() && h[p] == ' ') ++p;
    return p;
}
}  // namespace detail

// Parses `size` bytes of a .npy file.  Returns false and sets `err` on anything it does not accept.
inline bool parse(const uint8_t* bytes, size_t size, Array& out, std::string& err) {
    out.shape.clear();
    out.data.clear();
    static const uint8_t kMagic[6] = {0x93, 'N', 'U', 'M', 'P', 'Y'};
    if (size < 10 || std::memcmp(bytes, kMagic, 6) != 0) {
        err = "not a .npy file (bad magic or shorter than its preamble)";
        return false;
    }
    const unsigned major = bytes[6], minor = bytes[7];
    size_t headerLen, headerOff;
    if (major == 1 && minor == 0) {
        headerLen = (size_t)bytes[8] | ((size_t)bytes[9] << 8);
        headerOff = 10;
    } else if (major == 2 && minor == 0) {
        if (size < 12) {
            err = "truncated header";
            return false;
        }
        headerLen = (size_t)bytes[8] | ((size_t)bytes[9] << 8) | ((size_t)bytes[10] << 16) | ((size_t)bytes[11] << 24);
        headerOff = 12;
    } else {
        err = "unsupported .npy format version " + std::to_string(major) + "." + std::to_string(minor);
        return false;
    }
    if (headerLen > size - headerOff) {
        err = "truncated header";
        return false;
    }
    const std::string h((const char*)bytes + headerOff, headerLen);

    size_t p = detail::value_of(h, "descr");
    if (p == std::string::npos || p >= h.size() || (h[p] != '\'' && h[p] != '"')) {
        err = "header has no 'descr' string";
        return false;
    }
    const size_t q = h.find(h[p], p + 1);
    if (q == std::string::npos) {
        err = "header has no 'descr' string";
        return false;
    }
    const std::string descr = h.substr(p + 1, q - p - 1);
    if (descr != "<f4") {
        err = "dtype '" + descr + "' is not supported: only little-endian float32 ('<f4')";
        return false;
    }

    p = detail::value_of(h, "fortran_order");
    if (p == std::string::npos) {
        err = "header has no 'fortran_order'";
        return false;
    }
    if (h.compare(p, 5, "False") != 0) {
        err = "Fortran order is not supported: only C order";
        return false;
    }

    p = detail::value_of(h, "shape");
    if (p == std::string::npos || p >= h.size() || h[p] != '(') {
        err = "header has no 'shape' tuple";
        return false;
    }
    ++p;
    uint64_t count = 1;
    bool closed = false;
    while (p < h.size()) {
        while (p < h.size() && (h[p] == ' ' || h[p] == ',')) ++p;
        if (p < h.size() && h[p] == ')') {
            closed = true;
            break;
        }
        if (p >= h.size() || h[p] < '0' || h[p] > '9') break;
        uint64_t v = 0;
        while (p < h.size() && h[p] >= '0' && h[p] <= '9') {
            const uint64_t d = (uint64_t)(h[p] - '0');
            if (v > (UINT64_MAX - d) / 10) {
                err = "shape overflows";
                return false;
            }
            v = v * 10 + d;
            ++p;
        }
        if (p < h.size() && h[p] == 'L') ++p;  // Python 2 longs
        if (v != 0 && count > UINT64_MAX / v) {
            err = "shape overflows";
            return false;
        }
        count *= v;
        out.shape.push_back(v);
    }
    if (!closed || out.shape.size() > 32) {
        err = "malformed 'shape' tuple";
        out.shape.clear();
        return false;
    }
    const size_t payload = size - headerOff - headerLen;
    if (count > UINT64_MAX / 4 || count * 4 != (uint64_t)payload) {
        err = "shape holds " + std::to_string(count) + " float32 values, the file " + std::to_string(payload) +
              " payload bytes" + (count <= UINT64_MAX / 4 && count * 4 > (uint64_t)payload ? " (truncated)" : "");
        out.shape.clear();
        return false;
    }
    out.data.resize((size_t)count);
    if (count) std::memcpy(out.data.data(), bytes + headerOff + headerLen, (size_t)count * 4);  // little-endian hosts
    return true;
}

inline bool load(const std::string& path, Array& out, std::string& err) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) {
        err = "cannot open " + path;
        return false;
    }
    std::vector<uint8_t> bytes;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) {
        err = "cannot read " + path;
        return false;
    }
    if (!parse(bytes.data(), bytes.size(), out, err)) {
        err = path + ": " + err;
        return false;
    }
    return true;
}

}  // namespace rsd::npy
