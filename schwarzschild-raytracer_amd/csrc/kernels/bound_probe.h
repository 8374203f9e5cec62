// bound_probe.h - the culling bounds of geodesic.hip, one call per thread.
//
// Test only (lib/libsr_bnd.so, -DSR_BOUND_PROBE; tests/test_gpu_bounds.py):
// every kernel here calls one shipping device function on per-lane inputs and
// writes what it returned; nothing is restated. What the step loop keeps
// wave-uniform (the scene pointer, the object or slot index, the reach mask)
// is a kernel argument, so the wave-uniform loads and SGPR pins of the device
// functions see what they see in the real kernels: one launch per slot.
// Grids are whole 64-lane waves; the lanes past n leave at once, so a ballot
// counts the live lanes only (clearance_obj, clearance_tr and the test-ray
// loops consult their wave-mates).
//
// The entry points take no context: the packed scene image and the segment
// buffer as sr_debug_pack_scene returns them (the bytes sr_set_scene and
// sr_set_test_ray upload), host arrays of inputs and outputs. Each uploads,
// launches, synchronises and copies back; 0, -1 on bad arguments (an index
// outside the image's counts), -3 on a HIP error.
//
// Included inside geodesic.hip's anonymous namespace, after the functions it
// calls.
#ifdef SR_BOUND_PROBE

// a Hit as the probes return it: 8 words
struct sr_probe_hit {
    int32_t slot, face, key;
    float dist, p[3];
    int32_t pad;
};

__device__ __forceinline__ void probe_store(sr_probe_hit* __restrict__ out, int i, const Hit& h) {
    sr_probe_hit r;
    r.slot = h.slot;
    r.face = h.face;
    r.key = h.key;
    r.dist = h.dist;
    r.p[0] = h.p.x;
    r.p[1] = h.p.y;
    r.p[2] = h.p.z;
    r.pad = 0;
    out[i] = r;
}

#define SR_PROBE_LANE()                                        \
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);       \
    if (i >= n) return

// in: {o[3], d[3], max_lambda}
__global__ __launch_bounds__(64) void sr_probe_hit_all_kernel(const sr_dev_scene* __restrict__ sc,
                                                              const float* __restrict__ segs,
                                                              const float* __restrict__ in, int n,
                                                              sr_probe_hit* __restrict__ out) {
    SR_PROBE_LANE();
    const float* q = in + 7 * (size_t)i;
    probe_store(out, i, closest_hit_all(sc, segs, ld3(q), ld3(q + 3), q[6]));
}

// in: {o[3], d[3], seg}
__global__ __launch_bounds__(64) void sr_probe_hit_chord_kernel(const sr_dev_scene* __restrict__ sc,
                                                                const float* __restrict__ segs, uint32_t reach,
                                                                const float* __restrict__ in, int n,
                                                                sr_probe_hit* __restrict__ out) {
    SR_PROBE_LANE();
    const float* q = in + 7 * (size_t)i;
    probe_store(out, i, closest_hit_chord<false>(sc, segs, reach, ld3(q), ld3(q + 3), q[6]));
}

// in: {o[3], d[3], seg}; S as closest_hit_chord forms it
__global__ __launch_bounds__(64) void sr_probe_may_hit_kernel(const sr_dev_scene* __restrict__ sc, int k,
                                                              const float* __restrict__ in, int n,
                                                              int32_t* __restrict__ out) {
    SR_PROBE_LANE();
    const float* q = in + 7 * (size_t)i;
    const f3 o = ld3(q);
    const float seg = q[6];
    const float S = (fabsf(o.x) + fabsf(o.y) + fabsf(o.z)) + seg + 1.0f;
    out[i] = may_hit(sc->objs[k], o, ld3(q + 3), seg, S) ? 1 : 0;
}

// in: {A[3], B[3], perr}; j = 0: the black hole, as budget_event calls it
__global__ __launch_bounds__(64) void sr_probe_reach_kernel(const sr_dev_scene* __restrict__ sc, int j,
                                                            const float* __restrict__ in, int n,
                                                            int32_t* __restrict__ out) {
    SR_PROBE_LANE();
    const float* q = in + 7 * (size_t)i;
    bool r;
    if (j == 0) {
        r = slot_reachable(nullptr, 0, ld3(q), ld3(q + 3), q[6]);
    } else {
        const sr_dev_slot sl = pin_slot(sc->slots[j - 1]);
        r = slot_reachable(&sl, j, ld3(q), ld3(q + 3), q[6]);
    }
    out[i] = r ? 1 : 0;
}

// in: A[3]; a = |A| by the hardware square root, as budget_event forms it.
// j >= 1: clearance_obj of slot j; j = 0: clearance_bh
__global__ __launch_bounds__(64) void sr_probe_clear_kernel(const sr_dev_scene* __restrict__ sc, int j,
                                                            const float* __restrict__ in, int n,
                                                            float* __restrict__ out) {
    SR_PROBE_LANE();
    const f3 A = ld3(in + 3 * (size_t)i);
    const float a = __builtin_amdgcn_sqrtf(dot(A, A));
    if (j == 0) {
        out[i] = clearance_bh(a);
    } else {
        const sr_dev_slot sl = pin_slot(sc->slots[j - 1]);
        out[i] = clearance_obj(sl, A, a);
    }
}

// in: {A[3], dip, rlen}; not outward (an outward lane's shortcut is outward_clear's)
__global__ __launch_bounds__(64) void sr_probe_clear_tr_kernel(const sr_dev_scene* __restrict__ sc,
                                                               const float* __restrict__ segs,
                                                               const float* __restrict__ in, int n,
                                                               float* __restrict__ out, uint32_t* __restrict__ gm_out) {
    SR_PROBE_LANE();
    const float* q = in + 5 * (size_t)i;
    const f3 A = ld3(q);
    const float a = __builtin_amdgcn_sqrtf(dot(A, A));
    uint32_t gm;
    out[i] = clearance_tr(sc, segs, A, false, a, q[3], q[4], gm);
    gm_out[i] = gm;
}

// in: {ro[3], rd[3]}
__global__ __launch_bounds__(64) void sr_probe_flat_kernel(const sr_dev_scene* __restrict__ sc,
                                                           const float* __restrict__ in, int n,
                                                           int32_t* __restrict__ out) {
    SR_PROBE_LANE();
    const float* q = in + 6 * (size_t)i;
    out[i] = flat_misses(sc, ld3(q), ld3(q + 3)) ? 1 : 0;
}

// in: {u, up, r2, nv[3], tv[3], cos phi', sin phi', cos phi, sin phi}: (u, phi)
// after step i - 1, (up, phi') after step i - 2 in the orbital frame (nv, tv).
// out: {certain_end(u, up, r2), sphere_lambda_r2 on the chord settle_prev
// builds from them (ro = its end, rd = its direction), as the reseed calls it}
__global__ __launch_bounds__(64) void sr_probe_end_kernel(const float* __restrict__ in, int n,
                                                          int32_t* __restrict__ out) {
    SR_PROBE_LANE();
    const float* q = in + 13 * (size_t)i;
    const float u = q[0], up = q[1], r2 = q[2];
    Ray r = {};
    r.nv = ld3(q + 3);
    r.tv = ld3(q + 6);
    const f3 A = point_at(r, up, q[9], q[10]);
    const f3 B = point_at(r, u, q[11], q[12]);
    const f3 delta = B - A;
    const float seg = len(delta);
    const f3 rd = delta / seg;
    float lam;
    out[2 * i] = certain_end(u, up, r2) ? 1 : 0;
    out[2 * i + 1] = sphere_lambda_r2(B, rd, F3(0.0f, 0.0f, 0.0f), r2, -1.0f, lam) ? 1 : 0;
}

// ---- host side ---------------------------------------------------------------
// The image's counts index its arrays on the device: refuse one that could
// read outside them.
inline bool probe_image_ok(const sr_dev_scene* s) {
    if (!s) return false;
    if (s->num_objects < 0 || s->num_objects > SR_MAX_OBJECTS) return false;
    if (s->num_budget < 0 || s->num_budget > SR_MAX_BUDGET || s->num_budget > SR_MAX_OBJECTS) return false;
    if (s->num_step < 0 || s->num_step > SR_MAX_OBJECTS) return false;
    for (int j = 0; j < s->num_budget; j++)
        if (s->budget_idx[j] < 0 || s->budget_idx[j] >= s->num_objects) return false;
    for (int j = 0; j < s->num_step; j++)
        if (s->step_idx[j] < 0 || s->step_idx[j] >= s->num_objects) return false;
    if (s->tr_num_segments < 0 || s->tr_num_segments > SR_MAX_POINTS - 1) return false;
    if (s->tr_num_blocks < 0 || s->tr_num_blocks > SR_TR_BLOCKS) return false;
    if (s->tr_num_groups < 0 || s->tr_num_groups > SR_TR_GROUPS) return false;
    if (s->tr_num_blocks * SR_TR_BLOCK < s->tr_num_segments && s->tr_num_blocks > 0) return false;
    return true;
}

struct ProbeBuffers {
    sr_dev_scene* sc = nullptr;
    float* segs = nullptr;
    float* in = nullptr;
    void* out = nullptr;
    void* out2 = nullptr;
    ~ProbeBuffers() {
        (void)hipFree(sc);
        (void)hipFree(segs);
        (void)hipFree(in);
        (void)hipFree(out);
        (void)hipFree(out2);
    }
};

// Uploads the image, the segments and n rows of `width` floats, runs
// launch(buffers, blocks), copies out_bytes (and out2_bytes) back.
template <class Launch>
int probe_run(const void* scene, const float* segs, const float* in, int width, int n, void* out, size_t out_bytes,
              void* out2, size_t out2_bytes, Launch launch) {
    if (!scene || !segs || !in || !out || n < 0 || n > (1 << 20)) return -1;
    if (!probe_image_ok(static_cast<const sr_dev_scene*>(scene))) return -1;
    if (n == 0) return 0;
    ProbeBuffers b;
    const size_t seg_bytes = (size_t)SR_SEGS_BUF_FLOATS * sizeof(float);
    const size_t in_bytes = (size_t)n * (size_t)width * sizeof(float);
    if (hipMalloc(&b.sc, sizeof(sr_dev_scene)) != hipSuccess || hipMalloc(&b.segs, seg_bytes) != hipSuccess ||
        hipMalloc(&b.in, in_bytes) != hipSuccess || hipMalloc(&b.out, out_bytes) != hipSuccess)
        return -3;
    if (out2 && hipMalloc(&b.out2, out2_bytes) != hipSuccess) return -3;
    if (hipMemcpy(b.sc, scene, sizeof(sr_dev_scene), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b.segs, segs, seg_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b.in, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(b.out, 0, out_bytes) != hipSuccess)
        return -3;
    launch(b, dim3((unsigned)((n + 63) / 64)));
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpy(out, b.out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return -3;
    if (out2 && hipMemcpy(out2, b.out2, out2_bytes, hipMemcpyDeviceToHost) != hipSuccess) return -3;
    return 0;
}

extern "C" int sr_debug_probe_hit_all(const void* scene, const float* segs, const float* in, int n, void* out) {
    return probe_run(scene, segs, in, 7, n, out, (size_t)n * sizeof(sr_probe_hit), nullptr, 0,
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_hit_all_kernel, g, dim3(64), 0, 0, b.sc, b.segs, b.in, n,
                                            static_cast<sr_probe_hit*>(b.out));
                     });
}

// reach: bit 0 the black hole, bit j budget slot j; bits past the image's slots are dropped
extern "C" int sr_debug_probe_hit_chord(const void* scene, const float* segs, uint32_t reach, const float* in, int n,
                                        void* out) {
    if (!scene || !probe_image_ok(static_cast<const sr_dev_scene*>(scene))) return -1;
    const int nb = static_cast<const sr_dev_scene*>(scene)->num_budget;
    if (nb + 1 < 32) reach &= (1u << (nb + 1)) - 1u;
    return probe_run(scene, segs, in, 7, n, out, (size_t)n * sizeof(sr_probe_hit), nullptr, 0,
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_hit_chord_kernel, g, dim3(64), 0, 0, b.sc, b.segs, reach, b.in, n,
                                            static_cast<sr_probe_hit*>(b.out));
                     });
}

extern "C" int sr_debug_probe_may_hit(const void* scene, const float* segs, int k, const float* in, int n,
                                      int32_t* out) {
    if (!scene || !probe_image_ok(static_cast<const sr_dev_scene*>(scene))) return -1;
    if (k < 0 || k >= static_cast<const sr_dev_scene*>(scene)->num_objects) return -1;
    return probe_run(scene, segs, in, 7, n, out, (size_t)n * sizeof(int32_t), nullptr, 0,
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_may_hit_kernel, g, dim3(64), 0, 0, b.sc, k, b.in, n,
                                            static_cast<int32_t*>(b.out));
                     });
}

extern "C" int sr_debug_probe_reach(const void* scene, const float* segs, int j, const float* in, int n,
                                    int32_t* out) {
    if (!scene || !probe_image_ok(static_cast<const sr_dev_scene*>(scene))) return -1;
    if (j < 0 || j > static_cast<const sr_dev_scene*>(scene)->num_budget) return -1;
    return probe_run(scene, segs, in, 7, n, out, (size_t)n * sizeof(int32_t), nullptr, 0,
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_reach_kernel, g, dim3(64), 0, 0, b.sc, j, b.in, n,
                                            static_cast<int32_t*>(b.out));
                     });
}

// j >= 1: clearance_obj of budget slot j; j = 0: clearance_bh
extern "C" int sr_debug_probe_clear(const void* scene, const float* segs, int j, const float* in, int n, float* out) {
    if (!scene || !probe_image_ok(static_cast<const sr_dev_scene*>(scene))) return -1;
    if (j < 0 || j > static_cast<const sr_dev_scene*>(scene)->num_budget) return -1;
    return probe_run(scene, segs, in, 3, n, out, (size_t)n * sizeof(float), nullptr, 0,
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_clear_kernel, g, dim3(64), 0, 0, b.sc, j, b.in, n,
                                            static_cast<float*>(b.out));
                     });
}

extern "C" int sr_debug_probe_clear_tr(const void* scene, const float* segs, const float* in, int n, float* out,
                                       uint32_t* gm) {
    if (!gm) return -1;
    return probe_run(scene, segs, in, 5, n, out, (size_t)n * sizeof(float), gm, (size_t)n * sizeof(uint32_t),
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_clear_tr_kernel, g, dim3(64), 0, 0, b.sc, b.segs, b.in, n,
                                            static_cast<float*>(b.out), static_cast<uint32_t*>(b.out2));
                     });
}

extern "C" int sr_debug_probe_flat(const void* scene, const float* segs, const float* in, int n, int32_t* out) {
    return probe_run(scene, segs, in, 6, n, out, (size_t)n * sizeof(int32_t), nullptr, 0,
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_flat_kernel, g, dim3(64), 0, 0, b.sc, b.in, n,
                                            static_cast<int32_t*>(b.out));
                     });
}

// out: n x {certain_end, sphere_lambda_r2}
extern "C" int sr_debug_probe_end(const void* scene, const float* segs, const float* in, int n, int32_t* out) {
    return probe_run(scene, segs, in, 13, n, out, (size_t)n * 2 * sizeof(int32_t), nullptr, 0,
                     [&](ProbeBuffers& b, dim3 g) {
                         hipLaunchKernelGGL(sr_probe_end_kernel, g, dim3(64), 0, 0, b.in, n,
                                            static_cast<int32_t*>(b.out));
                     });
}

// The step loop charges a budget T * SR_PATH_SLACK < clearance: the radius of
// the ball a clearance covers is the clearance over this factor.
extern "C" float sr_debug_probe_path_slack(void) { return SR_PATH_SLACK; }

// Where the tests' reader of the packed image (tests/bound_cases.py LAYOUT)
// finds its fields, in 4-byte words: out[0 .. n), n <= 21; the count.
extern "C" int sr_debug_probe_layout(int32_t* out, int n) {
#define SR_W(T, f) (int32_t)(offsetof(T, f) / 4)
    const int32_t w[] = {
        SR_W(sr_dev_scene, num_objects), SR_W(sr_dev_scene, tr_visible),     SR_W(sr_dev_scene, tr_num_segments),
        SR_W(sr_dev_scene, tr_num_groups), SR_W(sr_dev_scene, tr_radius),    SR_W(sr_dev_scene, num_budget),
        SR_W(sr_dev_scene, budget_idx),  SR_W(sr_dev_scene, slots),          (int32_t)(sizeof(sr_dev_slot) / 4),
        SR_W(sr_dev_scene, num_step),    SR_W(sr_dev_scene, step_idx),       SR_W(sr_dev_scene, flat_miss_r2),
        SR_W(sr_dev_scene, objs),        (int32_t)(sizeof(sr_dev_obj) / 4),  SR_W(sr_dev_obj, kind),
        SR_W(sr_dev_obj, bc),            SR_W(sr_dev_obj, br),               SR_W(sr_dev_slot, rb),
        SR_W(sr_dev_slot, br),           SR_W(sr_dev_slot, bc),              (int32_t)SR_MAX_OBJECTS};
#undef SR_W
    const int m = (int)(sizeof w / sizeof w[0]);
    for (int i = 0; out && i < n && i < m; i++) out[i] = w[i];
    return m;
}

#undef SR_PROBE_LANE
#endif  // SR_BOUND_PROBE
