// Philox4x32-10, first output word: the counter-based generator of the sampling kernels (sampling.hip) and of the Griffin-Lim
// initial phase (griffinlim.hip).  key = (k0, k1) = the low / high word of an utterance's 64-bit seed, counter = (c0, c1, c2, c3);
// u = (x0 >> 8) * 2^-24 is the uniform draw both use (tests/sampling_ref.py: uniform_np).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mt2 {

__device__ __forceinline__ uint32_t philox_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

}  // namespace mt2
