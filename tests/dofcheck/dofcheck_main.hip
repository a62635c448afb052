// TEST-ONLY stand-alone program: the per-value arithmetic of csrc/dhaug_dof_math.h compiled for the HOST, so that it can run
// under AddressSanitizer + UBSan (tests/test_dof_cpu.py builds and runs it; nothing here is loaded into Python).  UBSan's
// float-cast-overflow check is the point: bin_of must not convert a value to int before it knows the value is in range.
//
//   dofcheck
// sweeps every fp32 value within 4 ulp of every integer from -182 to 182 (both signs of zero included), +-0, the smallest
// and largest denormals, +-FLT_MIN, +-1e30, +-FLT_MAX, +-inf and NaNs of both signs, compares bin and flags with a restatement
// in double precision (floor / ceil by sign instead of truncf), checks that the integer keys of the extremes order the sweep
// as the values themselves do and convert back bit for bit, prints "checked <n> values, <m> mismatches" and exits 1 on a
// mismatch.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dhaug_dof_math.h"

using namespace dhaug_dof;

namespace {

int restated(double x, int& flags) {
    if (std::isnan(x)) {
        flags = F_NAN;
        return -1;
    }
    if (std::isinf(x)) {
        flags = F_OUTSIDE | F_INF;
        return x < 0 ? 0 : 360;
    }
    const double t = x < 0 ? std::ceil(x) : std::floor(x);      // towards zero
    if (t > 180.0) {
        flags = F_OUTSIDE;
        return 360;
    }
    if (t < -180.0) {
        flags = F_OUTSIDE;
        return 0;
    }
    flags = 0;
    return (int)t + 180;
}

float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

}  // namespace

int main() {
    std::vector<float> v;
    for (int i = -182; i <= 182; ++i) {
        float up = (float)i, down = (float)i;
        v.push_back((float)i);
        for (int k = 0; k < 4; ++k) {
            up = std::nextafterf(up, INFINITY);
            down = std::nextafterf(down, -INFINITY);
            v.push_back(up);
            v.push_back(down);
        }
    }
    const float specials[] = {0.0f, from_bits(1u), from_bits(0x007fffffu), FLT_MIN, 1e30f, FLT_MAX, INFINITY, 0.5f, 0.999f, 180.5f,
                              180.9f, 181.0f};
    for (float s : specials) {
        v.push_back(s);
        v.push_back(-s);
    }
    v.push_back(from_bits(0x7fc00000u));
    v.push_back(from_bits(0xffc00000u));
    v.push_back(from_bits(0x7f800001u));
    long bad = 0;
    for (float a : v) {
        int f = -7, g = -7;
        const int b = bin_of(a, f), c = restated((double)a, g);
        if (b != c || f != g) {
            std::printf("mismatch at %.9g (bits %08x): bin %d flags %d, restated bin %d flags %d\n", (double)a, bits_of(a), b, f, c, g);
            ++bad;
        }
        if (!(f & F_NAN)) {
            if (b < 0 || b >= kBins) {
                std::printf("bin %d out of range at %.9g\n", b, (double)a);
                ++bad;
            }
            if (bits_of(key_value(order_key(a))) != bits_of(a)) {
                std::printf("key does not convert back at %.9g (bits %08x)\n", (double)a, bits_of(a));
                ++bad;
            }
        }
    }
    // the keys order the values as < does, with -0 below +0
    for (float a : v) {
        for (float b : {-181.0f, -0.0f, 0.0f, 12.5f, 180.0f}) {
            if (a != a) continue;
            const bool lt = a < b || (a == b && std::signbit(a) && !std::signbit(b));
            if ((order_key(a) < order_key(b)) != lt) {
                std::printf("key order differs for %.9g and %.9g\n", (double)a, (double)b);
                ++bad;
            }
        }
    }
    std::printf("checked %zu values, %ld mismatches\n", v.size(), bad);
    return bad ? 1 : 0;
}
