// sky.hpp — the one statement of get_bg's texture coordinates (u, v) of a
// direction (frag:830-834; sr.h "Ray maps"), shared by the kernels' get_bg and
// ray maps (geodesic.hip) and the host's sr_sky_uv (sr_api.cpp), so that they
// cannot drift.
//
// Arithmetic contract: binary32 in the order written, no
// contraction (compile users with -ffp-contract=off), correctly rounded
// division, and atan2 / asin as the binary64 function of the float arguments
// rounded once to binary32. The caller supplies those two as `A` and `S` (the
// kernel passes its out-of-line device functions, the host the libm ones),
// everything else is written here once.
#ifndef SR_SKY_HPP
#define SR_SKY_HPP

#if defined(__HIP__)
#define SR_SKY_FN __host__ __device__ inline
#else
#define SR_SKY_FN inline
#endif

namespace sr {

// frag:10, the shader's PI
constexpr float kSkyPi = 3.1415926535f;

// (u, v) of get_bg(dir): u = atan(dir.z, dir.x) / PI, + 2 when negative,
// * 0.5; v = asin(dir.y) / PI + 0.5. The direction is taken as it is (get_bg
// does not normalise): |dir.y| > 1 gives a NaN v, as the shader's asin does.
template <class Atan2, class Asin>
SR_SKY_FN void sky_uv(float x, float y, float z, Atan2 A, Asin S, float uv[2]) {
    float u = A(z, x) / kSkyPi;
    if (u < 0.0f) u += 2.0f;
    u *= 0.5f;
    uv[0] = u;
    uv[1] = S(y) / kSkyPi + 0.5f;
}

}  // namespace sr

#endif
