// projection.hpp — the one statement of a pixel's local ray direction L for
// every camera projection (sr.h "Projections"), shared by the integrate
// kernel's init_pixel (geodesic.hip) and the host's sr_projection_dir
// (sr_api.cpp), so that the two cannot drift.
//
// Arithmetic contract: binary32 in the order written, no
// contraction (compile users with -ffp-contract=off), correctly rounded
// division and square root, and sin / cos as the binary64 function of the
// float argument rounded once to binary32. The caller supplies those two as
// `S` and `C` (the kernel passes its out-of-line device functions, the host
// the libm ones), everything else is written here once.
#ifndef SR_PROJECTION_HPP
#define SR_PROJECTION_HPP

#include <math.h>

#include "sr/sr.h"

#if defined(__HIP__)
#define SR_PROJ_FN __host__ __device__ inline
#else
#define SR_PROJ_FN inline
#endif

namespace sr {

// frag:10, the shader's PI
constexpr float kProjPi = 3.1415926535f;

// The half angle a = fov / 360 * PI: the argument of the tan behind the
// pinhole's forward term (frag:859), and the angle uv = 1 spans in the
// angular projections.
SR_PROJ_FN float projection_half_angle(float fov) { return fov / 360.0f * kProjPi; }

// L of the pixel with uvv = (uv.x, uv.y * res_y / res_x) under PROJ
// (SR_PROJECTION_*). a: projection_half_angle(fov); ray_forward: 1 / tan(a)
// (read by the pinhole alone). Returns false when the pixel has no ray (the
// fisheye beyond th = PI, NaNs included); L is then left unwritten.
template <int PROJ, class Sin, class Cos>
SR_PROJ_FN bool projection_local_dir(float uvx, float uvy, float a, float ray_forward, Sin S, Cos C, float L[3]) {
    if (PROJ == SR_PROJECTION_EQUIRECT) {
        const float lon = uvx * a, lat = uvy * a;
        const float cl = C(lat);
        L[0] = cl * S(lon);
        L[1] = S(lat);
        L[2] = cl * C(lon);
        return true;
    }
    if (PROJ == SR_PROJECTION_FISHEYE) {
        const float rho = sqrtf(uvx * uvx + uvy * uvy);
        const float th = rho * a;
        if (!(th <= kProjPi)) return false;
        const float s = S(th);
        if (rho > 0.0f) {
            L[0] = s * (uvx / rho);
            L[1] = s * (uvy / rho);
            L[2] = C(th);
        } else {
            L[0] = 0.0f;
            L[1] = 0.0f;
            L[2] = 1.0f;
        }
        return true;
    }
    L[0] = uvx;  // SR_PROJECTION_RECTILINEAR, frag:861-863
    L[1] = uvy;
    L[2] = ray_forward;
    return true;
}

}  // namespace sr

#endif
