// shutter_div.h — the shutter resolve's division (shutter.hip): n div k for
// n < 2^16 and k in 1 .. 256 as one multiplication and a shift, for a k known
// only at run time. Plain C++ without a HIP header: the kernel and the host
// (sr_debug_shutter_div, which tests/test_shutter_host.py holds to the
// integer quotient for every operand) compile the same two functions.
//
// m = floor(2^24 / k) + 1, so m k = 2^24 + e with 0 < e <= k <= 2^8. Then
// n m / 2^24 = n / k + n e / (k 2^24), and n e < 2^24 keeps the second term
// below 1 / k: the floor is that of n / k (Granlund and Montgomery, "Division
// by invariant integers using multiplication", 1994, for N = 16 and l = 8).
// The product needs 41 bits.
#ifndef SR_KERNELS_SHUTTER_DIV_H
#define SR_KERNELS_SHUTTER_DIV_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_DIV_FN __host__ __device__ inline
#else
#define SR_DIV_FN inline
#endif

SR_DIV_FN uint32_t sr_shutter_magic(uint32_t k) { return (1u << 24) / k + 1u; }
SR_DIV_FN uint32_t sr_shutter_div(uint32_t n, uint32_t magic) { return (uint32_t)(((uint64_t)n * magic) >> 24); }

#endif
