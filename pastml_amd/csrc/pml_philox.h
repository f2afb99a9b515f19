// Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator of the
// scenario sampler (pml_kernels_counts.h) and of the forward simulator (pml_kernels_simulate.h).  A draw is a pure function
// of (key, counter), so results do not depend on the launch geometry.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox4x32_10(unsigned (&ctr)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * ctr[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * ctr[2];
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0;
        const unsigned hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        const unsigned n0 = hi1 ^ ctr[1] ^ k0, n1 = lo1, n2 = hi0 ^ ctr[3] ^ k1, n3 = lo0;
        ctr[0] = n0;
        ctr[1] = n1;
        ctr[2] = n2;
        ctr[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
