// precompute.h — the host arithmetic the "exact by margin" culling rests on:
// the scene image (bounds, budget slots, the test ray's segments and their
// culling bounds), a frame's derived constants, the low-energy exclusions, the
// step table, the opacity bitmap and the first launch order. Plain C++ with no
// HIP header and no context: the C ABI (sr_api.cpp) packs through these
// functions and uploads what they return; the sr_debug_* exports and the CPU
// tests call the same functions. Float-exact code: built with
// -ffp-contract=off like the kernels.
#ifndef SR_HOST_PRECOMPUTE_H
#define SR_HOST_PRECOMPUTE_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "device_scene.h"
#include "sr/sr.h"

namespace sr_pre {

// The scene part of the image from `s` (objects, bounds, budget slots, the
// far-field miss radius, materials, lights); the test-ray part of `d` stays.
// SR_E_INVALID / SR_E_CAPACITY as sr_set_scene; `d` is then partly written.
int pack_scene(const sr_scene& s, sr_dev_scene& d);

// The test-ray part of the image and the segment buffer (SR_SEGS_BUF_FLOATS
// floats: the segments, then their block and group bounds); the scene part of
// `d` stays. SR_E_CAPACITY ahead of any write.
int pack_test_ray(const sr_test_ray& t, sr_dev_scene& d, std::vector<float>& segs);

// A launch's rejections of its camera, params and frame size (SR_E_INVALID)
int check_frame_args(const sr_camera* cam, const sr_params* p, int width, int height);

// What a launch's frame struct takes from its arguments and the scene alone
struct FrameInputs {
    const sr_camera* cams;  // n_frames cameras, or one for every frame of a phase launch (phase_cams unset)
    int n_frames;
    const sr_params* params;
    int width, height;
    int grid;               // the uv grid of a phase launch (phases set), else 1
    const uint8_t* phases;  // n_frames byte pairs {x, y}, or null
    bool cull;
    int projection;
    // a phase launch whose frame f has the camera cams[f] (sr.h "Shutter frames"), not cams[0]
    bool phase_cams = false;
};
// Zeroes `fr` and sets the cameras, the schedule's constants and margins
// (xplane_s, out_dip, max_dphi, bh_u2 / bh_u3, win_ok), the cull-off
// premises and the scene's slot counts; the exclusions are +inf / -1 (no
// exclusion). The rows, the output layout and the context's settings are the
// caller's. The arguments passed check_frame_args.
void derive_frame(const FrameInputs& in, const sr_dev_scene& sc, sr_dev_frame& fr);

// xlow_need and xperi_e of every budget slot for a (u_f, step angle) pair
void low_energy_exclusions(const sr_dev_scene& sc, float u_f, float max_dphi, float need[SR_MAX_BUDGET],
                           float peri[SR_MAX_BUDGET]);

// One step of the schedule, in the layout of the kernel's float4 loads
struct StepEntry {
    float step, step_sixth, cos_phi, sin_phi;
};
// max_steps entries and four of zero padding
std::vector<StepEntry> step_table(int max_steps, int max_revolutions);

// The texture array's opacity bitmap (geodesic.hip hit_opacity): rows of
// ceil(w / 8) bytes per texel row per layer
std::vector<uint8_t> opacity_bits(const uint8_t* px, int w, int h, int layers, int ch);

// The launch codes of a gx x gy grid before any frame has measured its costs:
// whole tiles nearest the frame centre first, then -1 up to `slots`
std::vector<int> centre_first_order(int gx, int gy, size_t slots);

}  // namespace sr_pre

#endif
