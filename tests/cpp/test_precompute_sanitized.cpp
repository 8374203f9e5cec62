// Runs csrc/host/precompute.cpp, linked directly and built with
// -fsanitize=address,undefined (tests/test_host_precompute.py), over inputs at
// its limits: every sr_scene of the file given as argv[1] (the max-capacity
// scene and the non-finite ones of tests/extreme_cases.py, written by the
// test), a 1000-point test ray, frames at u_f = 0, NaN and +inf, the largest
// step table and a 1 x 1 and an odd-sized texture array. Prints ALL OK.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host/precompute.h"

static int fail(const char* what, int rc) {
    std::printf("FAILED: %s (%d)\n", what, rc);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: test_precompute_sanitized SCENES.bin", 0);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the scene file", 0);
    std::vector<sr_scene> scenes;
    sr_scene s;
    while (std::fread(&s, sizeof s, 1, f) == 1) scenes.push_back(s);
    std::fclose(f);
    if (scenes.empty()) return fail("no scene in the file", 0);

    // a 1000-point polyline: a spiral through the origin's neighbourhood, its last point inside r = 1
    static sr_test_ray t;
    std::memset(&t, 0, sizeof t);
    t.visible = 1;
    t.radius = 0.05f;
    t.extended_length = 50.0f;
    t.flat_origin[2] = 15.0f;
    t.flat_dir[0] = 0.1f, t.flat_dir[1] = -0.2f, t.flat_dir[2] = -1.0f;
    t.num_curved_points = SR_MAX_POINTS;
    for (int i = 0; i < SR_MAX_POINTS; i++) {
        const float a = 0.02f * (float)i, r = 20.0f * (1.0f - (float)i / (float)SR_MAX_POINTS) + 0.5f;
        t.curved_points[i][0] = r * std::cos(a);
        t.curved_points[i][1] = 0.3f * std::sin(3.0f * a);
        t.curved_points[i][2] = r * std::sin(a);
    }

    sr_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.transform.pos[1] = 2.0f, cam.transform.pos[2] = 15.0f;
    cam.transform.axes[0] = cam.transform.axes[4] = 1.0f, cam.transform.axes[8] = -1.0f;
    cam.fov = 90.0f;
    const float ufs[3] = {0.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};

    static sr_dev_scene d;
    std::vector<float> segs;
    size_t budgeted = 0;
    for (size_t k = 0; k < scenes.size(); k++) {
        std::memset(&d, 0, sizeof d);
        d.flat_miss_r2 = INFINITY;
        int rc = sr_pre::pack_test_ray(t, d, segs);
        if (rc != SR_OK || segs.size() != (size_t)SR_SEGS_BUF_FLOATS) return fail("pack_test_ray", rc);
        if (d.tr_num_segments != SR_MAX_POINTS - 1 || d.tr_num_blocks != SR_TR_BLOCKS || d.tr_num_groups != SR_TR_GROUPS)
            return fail("the test ray's segment counts", d.tr_num_segments);
        rc = sr_pre::pack_scene(scenes[k], d);
        if (rc != SR_OK) return fail("pack_scene", rc);
        if (d.num_budget + d.num_step != scenes[k].num_objects) return fail("slot counts", d.num_budget);
        budgeted += (size_t)d.num_budget;
        for (float u_f : ufs) {
            sr_params p;
            std::memset(&p, 0, sizeof p);
            p.max_steps = 400;
            p.max_revolutions = 2;
            p.u_f = u_f;
            rc = sr_pre::check_frame_args(&cam, &p, 68, 44);
            if (rc != SR_OK) return fail("check_frame_args", rc);
            static sr_dev_frame fr;
            sr_pre::derive_frame({&cam, 1, &p, 68, 44, 1, nullptr, true, SR_PROJECTION_RECTILINEAR}, d, fr);
            sr_pre::low_energy_exclusions(d, fr.u_f, fr.max_dphi, fr.xlow_need, fr.xperi_e);
            if (fr.batch != 1 || fr.num_budget != d.num_budget) return fail("derive_frame", fr.batch);
            if (std::isnan(u_f) && fr.cull != 0) return fail("a NaN u_f keeps culling on", fr.cull);
        }
    }
    if (budgeted == 0) return fail("no scene has a budgeted object", 0);

    if (sr_pre::step_table(SR_MAX_STEPS, 3).size() != (size_t)SR_MAX_STEPS + 4) return fail("step_table", 0);
    if (sr_pre::step_table(0, 0).size() != 4) return fail("the empty step table", 0);
    const uint8_t one[4] = {1, 2, 3, 255};
    if (sr_pre::opacity_bits(one, 1, 1, 1, 4) != std::vector<uint8_t>{1}) return fail("opacity_bits 1x1", 0);
    std::vector<uint8_t> px((size_t)2 * 5 * 13 * 4, 255);
    px[3] = 0;
    if (sr_pre::opacity_bits(px.data(), 13, 5, 2, 4).size() != 2 * 5 * 2) return fail("opacity_bits 13x5x2", 0);
    if (sr_pre::opacity_bits(px.data(), 13, 5, 2, 3).size() != 2 * 5 * 2) return fail("opacity_bits rgb", 0);
    if (sr_pre::centre_first_order(5, 3, 15 + 63 * 4).size() != 15 + 63 * 4) return fail("centre_first_order", 0);
    std::printf("ALL OK: %zu scenes\n", scenes.size());
    return 0;
}
