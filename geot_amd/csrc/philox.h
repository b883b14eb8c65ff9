// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator of
// geot_sample_draw and geot_view_draw.  Four counter words, two key words, ten rounds, the key bumped by the Weyl constants
// between rounds; integer arithmetic only, the same on the host and on the device.
#pragma once
#include <stdint.h>

#ifndef GEOT_HD
#ifdef __HIPCC__
#define GEOT_HD __host__ __device__ __forceinline__
#else
#define GEOT_HD inline
#endif
#endif

namespace geot {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct Philox4 {
    uint32_t w[4];
};

GEOT_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0, p1 = (unsigned long long)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

} // namespace geot
