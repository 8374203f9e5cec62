// sr_api.cpp — the C-ABI of include/sr/sr.h: the device context (stream
// ordering, its caches, grow-on-demand scratch), texture and scene uploads and
// kernel dispatch. The launch-invariant arithmetic is host/precompute.cpp's
// (no HIP; the CPU tests call it), the kernel launchers are declared in
// kernels/launchers.h and nowhere else.
// Replaces the reference's GL program interface: the draw call of
// src/main.cpp:318-319 becomes sr_render, the loadShader uniform uploads
// become sr_set_scene / sr_set_test_ray snapshots.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <tuple>
#include <utility>
#include <vector>

#include "device_scene.h"
#include "host/device_cache.h"
#include "host/precompute.h"
#include "kernels/launchers.h"
#include "kernels/shutter_div.h"
#include "sr/projection.hpp"
#include "sr/sky.hpp"
#include "sr/sr.h"

static_assert(sizeof(sr_pre::StepEntry) == sizeof(float4), "a step-table entry is one float4 load of the kernel");

namespace {

// A grow-on-demand scratch buffer of the context (grow, drop), `n` elements:
// the pixel pipeline's SR_PS_FIELDS planes of floats per pixel id, resume
// worklist and counter pair (geodesic.hip); the sample frame of a supersampled
// launch (resolve.hip); adaptive supersampling's flagged output tiles (bytes)
// and the sparse launch's code list (adaptive.hip)
struct Scratch {
    void* p = nullptr;
    size_t n = 0;
};
enum { kPs, kList, kCount, kSs, kAmask, kAcodes, kScratches };

}  // namespace

struct sr_ctx {
    int device = 0;
    sr_dev_scene* d_scene = nullptr;
    float* d_segs = nullptr;
    uint32_t* d_bg = nullptr;
    int bg_w = 0, bg_h = 0;
    uint32_t* d_arr = nullptr;
    int arr_w = 0, arr_h = 0, arr_layers = 0;
    uint8_t* d_opq = nullptr;  // texture-array opacity bitmap (precompute.cpp opacity_bits)
    bool scene_set = false;
    bool cull = true;
    sr_dev_scene h_scene;
    // low_energy_exclusions' last inputs and results (build_frame; cleared by sr_set_scene)
    float xc_uf = NAN, xc_dphi = NAN;
    float xc_need[SR_MAX_BUDGET];
    float xc_peri[SR_MAX_BUDGET];
    // reused per frame (renders on one context are ordered on its stream(s)
    // by the caller); ps_n: the pixel ids the pixel state holds
    Scratch scratch[kScratches];
    size_t ps_n() const { return scratch[kList].n; }
    float* d_ps() const { return static_cast<float*>(scratch[kPs].p); }
    int* d_list() const { return static_cast<int*>(scratch[kList].p); }
    int* d_count() const { return static_cast<int*>(scratch[kCount].p); }
    uint8_t* d_ss() const { return static_cast<uint8_t*>(scratch[kSs].p); }
    uint8_t* d_amask() const { return static_cast<uint8_t*>(scratch[kAmask].p); }
    int* d_acodes() const { return static_cast<int*>(scratch[kAcodes].p); }
    // step tables, the sequence's exclusion tables, launch orders, block lists
    // and the launch codes of the context's last frame (its next frame's order).
    // An entry goes in stream order or, with the sequence, after a wait.
    sr_cache::Caches caches;
    // synchronous uploads (sr_set_*) run on this non-blocking stream, never
    // on the null stream (which would wait for other contexts' work)
    hipStream_t upload = nullptr;
    // split tiles (sr_set_split): 0 = off
    int split_tiles = 0, split_log2 = 4, split_min_steps = 1;
    int fast_unroll = SR_FAST_UNROLL_DEFAULT;  // sr_set_latency_mode: 2
    int projection = SR_PROJECTION_RECTILINEAR;  // sr_set_projection
    // the stream of the context's last launch: a context is used from one
    // stream, so waiting for it waits for every frame that
    // may still read the context's buffers, and for nothing else on the device
    hipStream_t last_stream = nullptr;
    bool launched = false;
    // a launch on another stream than the last one first waits for it (this
    // event, recorded on the old stream): the context's scratch and the
    // stream-ordered frees on last_stream stay ordered after every launch
    hipEvent_t order_ev = nullptr;
    // stream-ordered frees whose hipFreeAsync failed (sr_diag_counters)
    int64_t free_errors = 0;
    // device counter of the shade kernel's invariant check (sr_diag_counters)
    int* d_diag = nullptr;
    // the start table: one record per frame of a batch, rebuilt by every
    // launch on its stream before the integrate kernel reads it (geodesic.hip
    // sr_start_table_kernel); nothing in it outlives the launch
    sr_dev_start* d_start = nullptr;
    // optional per-kernel timing: 4 events per frame (before integrate, after
    // integrate, after shade, after resume), a ring of `timing_cap` frames
    std::vector<hipEvent_t> tev;
    int timing_cap = 0;
    int timing_n = 0;
    // the retained frame (sr.h "Retained frames"): what the pixel state holds
    // since the last launch, for sr_reshade and sr_pick_map. fr is the
    // launch's own frame struct (a supersampled launch's: the sample frame's);
    // the step table is re-ensured from its key. ss > 1: the resolve's
    // arguments, in output pixels.
    struct Retained {
        bool valid = false;
        sr_dev_frame fr;
        int max_steps = 0, max_revolutions = 0;
        int ss = 1;
        int width = 0, height = 0, rows = 0, block_rows = 0;
        const int* d_blocks = nullptr;
    } kept;
    // the scene of the last successful sr_set_scene (sr_scene_shading_only's left side)
    sr_scene scene_src;
    // the scene sequence (sr.h "Scene sequences"): its images as one device
    // array and their host copies (sr_set_test_ray packs their test-ray part
    // again); a state of its own beside d_scene / h_scene
    sr_dev_scene* d_seq = nullptr;
    std::vector<sr_dev_scene> h_seq;
};

namespace {

inline bool hip_ok(hipError_t e) { return e == hipSuccess; }
inline int status(hipError_t e) { return hip_ok(e) ? SR_OK : SR_E_HIP; }

// Frees a device buffer in stream order: after the context's in-flight
// frames (its last launch stream; `s` before its first launch). hipFree would
// synchronise the whole device.
void release(sr_ctx* ctx, void* p, hipStream_t s) {
    if (p && !hip_ok(hipFreeAsync(p, ctx->launched ? ctx->last_stream : s))) ctx->free_errors++;
}

// The caches' device (host/device_cache.h); the frees are release()'s
struct HipDevice {
    sr_ctx* ctx;
    bool alloc(void** p, size_t bytes, void* s) { return hip_ok(hipMallocAsync(p, bytes, hipStream_t(s))); }
    bool upload(void* dst, const void* src, size_t bytes, void* s) {
        return hip_ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, hipStream_t(s)));
    }
    bool zero(void* dst, size_t bytes, void* s) { return hip_ok(hipMemsetAsync(dst, 0, bytes, hipStream_t(s))); }
    void free(void* p, void* s) { release(ctx, p, hipStream_t(s)); }
};

int ensure_table(sr_ctx* ctx, int max_steps, int max_revs, hipStream_t s, const float4** out) {
    return ctx->caches.table(
        HipDevice{ctx}, {max_steps, max_revs}, s, ctx->last_stream,
        [&](std::vector<sr_pre::StepEntry>& t) { t = sr_pre::step_table(max_steps, max_revs); }, out);
}

// Floats per scene of an exclusion table (geodesic.hip SR_XTAB_FLOATS)
constexpr size_t kXTabFloats = 2 * SR_MAX_BUDGET;

// The sequence's exclusion table for a launch's (u_f, step angle): xlow_need,
// then xperi_e, of every scene, as sr_launch_geodesic_seq reads them
int ensure_xtab(sr_ctx* ctx, float u_f, float max_dphi, hipStream_t s, const float** out) {
    return ctx->caches.xtab(
        HipDevice{ctx}, u_f, max_dphi, s, ctx->last_stream,
        [&](std::vector<float>& t) {
            t.resize(ctx->h_seq.size() * kXTabFloats);
            for (size_t k = 0; k < ctx->h_seq.size(); k++)
                sr_pre::low_energy_exclusions(ctx->h_seq[k], u_f, max_dphi, &t[k * kXTabFloats],
                                              &t[k * kXTabFloats + SR_MAX_BUDGET]);
        },
        out);
}

// Synchronous upload of host bytes into a fresh device buffer on the
// context's private upload stream (the previous buffer is freed in stream
// order after the context's in-flight frames).
int upload_bytes(sr_ctx* ctx, const void* src, size_t bytes, void** dev) {
    release(ctx, *dev, ctx->upload);
    *dev = nullptr;
    if (!hip_ok(hipMallocAsync(dev, bytes, ctx->upload))) return SR_E_NOMEM;
    if (!hip_ok(hipMemcpyAsync(*dev, src, bytes, hipMemcpyHostToDevice, ctx->upload)) ||
        !hip_ok(hipStreamSynchronize(ctx->upload)))
        return SR_E_HIP;
    return SR_OK;
}

int upload_rgba(sr_ctx* ctx, const uint8_t* px, int w, int h, int layers, int ch, uint32_t** dev) {
    size_t n = (size_t)w * h * layers;
    std::vector<uint32_t> rgba(n);
    for (size_t i = 0; i < n; i++) {
        const uint8_t* p = px + i * ch;
        uint32_t a = ch == 4 ? p[3] : 255u;  // GL_RGB reads alpha 1
        rgba[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | (a << 24);
    }
    return upload_bytes(ctx, rgba.data(), n * sizeof(uint32_t), reinterpret_cast<void**>(dev));
}

// Waits for this context's in-flight frames (its last launch stream), not
// for the device: other contexts' frames and collectives run on.
bool wait_ctx(sr_ctx* ctx) {
    if (!ctx->launched) return true;
    return hip_ok(hipStreamSynchronize(ctx->last_stream));
}

void drop(sr_ctx* ctx, Scratch& b, hipStream_t s) {
    release(ctx, b.p, s);
    b = Scratch();
}

// Grows a scratch buffer to `want` elements of `size` bytes in stream order:
// the old buffer is freed after the context's in-flight frames, the new one
// allocated on the caller's stream ahead of the launch (no host wait, no
// device-wide synchronisation); its contents are not kept.
int grow(sr_ctx* ctx, int which, size_t want, size_t size, hipStream_t s) {
    Scratch& b = ctx->scratch[which];
    if (want <= b.n) return SR_OK;
    drop(ctx, b, s);
    if (!hip_ok(hipMallocAsync(&b.p, want * size, s))) {
        b.p = nullptr;
        return SR_E_NOMEM;
    }
    b.n = want;
    return SR_OK;
}

void free_pixel_state(sr_ctx* ctx, hipStream_t s) {
    ctx->kept.valid = false;  // the retained rays go with the planes
    for (int b : {kPs, kList, kCount}) drop(ctx, ctx->scratch[b], s);
}

// Grows the pixel state to n pixel ids
int ensure_pixel_state(sr_ctx* ctx, size_t n, hipStream_t s) {
    if (n <= ctx->ps_n()) return SR_OK;
    free_pixel_state(ctx, s);
    int rc = grow(ctx, kPs, n * SR_PS_FIELDS, sizeof(float), s);
    if (rc == SR_OK) rc = grow(ctx, kList, n, sizeof(int), s);
    if (rc == SR_OK) rc = grow(ctx, kCount, 2, sizeof(int), s);
    // [0]: the shade kernel's resume queue
    if (rc == SR_OK) rc = status(hipMemsetAsync(ctx->d_count(), 0, 2 * sizeof(int), s));
    if (rc != SR_OK) free_pixel_state(ctx, s);
    return rc;
}

// Entries of a launch order over n tiles: the split grid adds (64 >> log2) - 1
// workgroups for each of its split_tiles tiles (geodesic.hip order_tiles)
size_t launch_slots(const sr_ctx* ctx, size_t n) {
    const int split = ctx->split_tiles;
    return n + (size_t)((64 >> (split ? ctx->split_log2 : 6)) - 1) * (size_t)split;
}

// Launch order for a grid shape: tiles nearest the frame centre first (where
// the black hole usually is) until a frame has measured the costs. One
// buffer pair per shape and split setting, allocated on first use. Entries
// are launch codes (geodesic.hip order_tiles): tile << 8 for a whole
// tile, -1 for the split grid's slots no tile uses yet. out[0]: the order,
// out[1]: the tiles' costs.
int ensure_order(sr_ctx* ctx, int gx, int gy, const int* list, hipStream_t s, int** out) {
    const int split = ctx->split_tiles;
    const size_t n = (size_t)gx * gy;
    return ctx->caches.order(
        HipDevice{ctx}, std::make_tuple(gx, gy, split, split ? ctx->split_log2 : 0, list, ctx->projection),
        n * sizeof(int), s, ctx->last_stream,
        [&](std::vector<int>& o) { o = sr_pre::centre_first_order(gx, gy, launch_slots(ctx, n)); }, out);
}

// The block-list paths' own rejections: the arguments, the rows of the launch
// (ss x the list's, at most 2^24) and every index (-1: padding).
int check_block_list(const sr_ctx* c, const void* out, const int* blocks, int n_blocks, int block_rows, int height,
                     int ss) {
    if (!c || !out || !blocks || block_rows <= 0 || n_blocks <= 0 || height <= 0) return SR_E_INVALID;
    if ((long long)ss * n_blocks * block_rows > (1 << 24)) return SR_E_INVALID;
    const int nb = (height + block_rows - 1) / block_rows;
    for (int i = 0; i < n_blocks; i++)
        if (blocks[i] < -1 || blocks[i] >= nb) return SR_E_INVALID;
    return SR_OK;
}

// The device copy of a block list, uploaded once per distinct list (a rank's
// balanced list does not change between frames); after enter_stream, like every ensure_*.
int ensure_block_list(sr_ctx* ctx, const int* blocks, int n, hipStream_t s, const int** dev) {
    const sr_ctx::Retained& k = ctx->kept;
    const int* const kept[2] = {k.valid ? k.fr.block_list : nullptr, k.valid ? k.d_blocks : nullptr};
    bool gone = false;
    const int rc = ctx->caches.block_list(HipDevice{ctx}, blocks, n, s, ctx->last_stream, kept, &gone, dev);
    if (gone) ctx->kept.valid = false;
    return rc;
}

// Makes `s` the context's launch stream: ordered after the launches on the
// previous one, and the target of every stream-ordered free from here on
// (ensure_*'s evictions).
int enter_stream(sr_ctx* ctx, hipStream_t s) {
    if (!hip_ok(hipSetDevice(ctx->device))) return SR_E_HIP;
    if (ctx->launched && s != ctx->last_stream) {
        // order_ev was recorded at the end of the last launch, so the old
        // stream's handle is not touched here (the caller may have destroyed
        // it since)
        if (!hip_ok(hipStreamWaitEvent(s, ctx->order_ev, 0))) return SR_E_HIP;
    }
    ctx->last_stream = s;
    return SR_OK;
}

// The end of everything an entry point put on `s`: the event a launch on
// another stream will wait for (enter_stream), and the status.
int finish(sr_ctx* ctx, hipError_t e, hipStream_t s) {
    if (hip_ok(e)) e = hipEventRecord(ctx->order_ev, s);
    ctx->launched = true;
    return status(e);
}

inline bool bad_rows(int row_begin, int row_end, int height) {
    return row_begin < 0 || row_end > height || row_begin > row_end;
}

// One launch of each kernel: the same rows of n_frames frames (cams[f]; output
// f at out + f * frame_stride).
struct Launch {
    // frames
    const sr_camera* cams = nullptr;
    int n_frames = 1;
    const sr_params* params = nullptr;
    int width = 0, height = 0;
    // rows: output row k renders frame row row_base + (k / block_rows) *
    // block_stride + k % block_rows, or the block list's (device_scene.h)
    int nrows = 0, row_base = 0, block_rows = 1, block_stride = 0;
    // the caller's list, and its device copy once resolved (ensure_block_list: after every rejection)
    const int* blocks = nullptr;
    int n_blocks = 0;
    const int* d_block_list = nullptr;
    // output
    uint8_t* out = nullptr;
    size_t pitch = 0, frame_stride = 0;
    float* dbg_rgba = nullptr;
    int32_t* dbg_steps = nullptr;
    // sr_wave_costs: per-wave costs instead of pixels
    int32_t* d_wave_cost = nullptr;
    // a sparse launch of one frame (sr_render_adaptive): the integrate and
    // shade kernels run the tiles of this device list of launch codes (one
    // entry per tile of the grid, -1 = none); no order of the grid's shape is
    // looked up, learned or updated, and split tiles do not apply to it
    int* d_codes = nullptr;
    // a phase launch (sr.h "Sample phases"; n_frames byte pairs {x, y}, each
    // in 0 .. grid - 1): every frame has the camera cams[0], frame f is phase
    // (phases[2 f], phases[2 f + 1]) of the grid x grid sample grid; width,
    // height and the rows are the output frame's
    int grid = 1;
    const uint8_t* phases = nullptr;
    // the sub-frames of shutter frames (sr.h "Shutter frames"): a phase launch
    // whose frame f has the camera cams[f], and under a sequence its scene
    bool phase_cams = false;
    // a sequence launch (sr.h "Scene sequences"; -1: none): frame f renders
    // scene seq_first + f of the context's sequence, not its own scene
    int seq_first = -1;
    sr_stream stream = nullptr;

    Launch() = default;
    Launch(const sr_camera* c, int n, const sr_params* p, int w, int h, sr_stream s)
        : cams(c), n_frames(n), params(p), width(w), height(h), stream(s) {}
    // rows [row_begin, row_begin + n) as one block
    Launch& band(int row_begin, int n) {
        nrows = n;
        row_base = row_begin;
        block_rows = n > 0 ? n : 1;
        block_stride = 0;
        return *this;
    }
    // blocks block_first, block_first + block_step, ... of block_rows rows (sr_render_blocks)
    Launch& strided_blocks(int rows_per_block, int block_first, int block_step) {
        int nblocks = 0;
        for (int b = block_first; b * rows_per_block < height; b += block_step) nblocks++;
        nrows = nblocks * rows_per_block;
        row_base = block_first * rows_per_block;
        block_rows = rows_per_block;
        block_stride = block_step * rows_per_block;
        return *this;
    }
    // the blocks of a list, -1 entries unwritten
    Launch& block_list(const int* list, int n, int rows_per_block) {
        nrows = n * rows_per_block;
        row_base = 0;
        block_rows = block_stride = rows_per_block;
        blocks = list;
        n_blocks = n;
        return *this;
    }
    Launch& sequence(int first_scene) {
        seq_first = first_scene < 0 ? INT32_MIN : first_scene;  // a negative index is rejected, not "none"
        return *this;
    }
    Launch& into(uint8_t* dev_out, size_t pitch_bytes, size_t frame_stride_bytes = 0) {
        out = dev_out;
        pitch = pitch_bytes;
        frame_stride = frame_stride_bytes;
        return *this;
    }
};

// A launch's rejections of the context and its frames, ahead of any allocation
// (seq_first: Launch::seq_first; a sequence launch needs the sequence, not sr_set_scene)
int check_frames(const sr_ctx* c, const sr_camera* cams, int n_frames, const sr_params* p, int width, int height,
                 int seq_first = -1) {
    if (!c) return SR_E_INVALID;
    if (seq_first == -1 ? !c->scene_set : c->h_seq.empty()) return SR_E_NOT_READY;
    if (!cams || n_frames < 1) return SR_E_INVALID;
    if (seq_first != -1 && (seq_first < 0 || (size_t)seq_first + (size_t)n_frames > c->h_seq.size())) return SR_E_INVALID;
    if (n_frames > SR_MAX_BATCH) return SR_E_CAPACITY;
    return sr_pre::check_frame_args(cams, p, width, height);
}

// What a frame struct takes from the context: its scene's low-energy
// exclusions per (u_f, step angle) (NaN: sr_set_scene's reset) and the texture sizes
void context_into_frame(sr_ctx* ctx, bool own_scene, sr_dev_frame& fr) {
    if (own_scene) {
        if (!(ctx->xc_uf == fr.u_f && ctx->xc_dphi == fr.max_dphi)) {
            sr_pre::low_energy_exclusions(ctx->h_scene, fr.u_f, fr.max_dphi, ctx->xc_need, ctx->xc_peri);
            ctx->xc_uf = fr.u_f;
            ctx->xc_dphi = fr.max_dphi;
        }
        std::memcpy(fr.xlow_need, ctx->xc_need, sizeof fr.xlow_need);
        std::memcpy(fr.xperi_e, ctx->xc_peri, sizeof fr.xperi_e);
    }
    fr.bg_w = ctx->bg_w;
    fr.bg_h = ctx->bg_h;
    fr.arr_w = ctx->arr_w;
    fr.arr_h = ctx->arr_h;
    fr.arr_layers = ctx->arr_layers;
}

// A launch's frame struct: every rejection, then the constants (precompute.cpp
// derive_frame, the low-energy exclusions per (u_f, step angle)), the
// context's settings and the request's rows. No HIP call.
int build_frame(sr_ctx* ctx, const Launch& r, sr_dev_frame& fr) {
    const int rc = check_frames(ctx, r.cams, r.n_frames, r.params, r.width, r.height, r.seq_first);
    if (rc != SR_OK) return rc;
    const bool seq = r.seq_first != -1;
    if (seq && (r.d_codes || r.d_wave_cost)) return SR_E_INVALID;
    if (r.phases) {
        if (r.grid < 1 || r.grid > SR_MAX_SUPERSAMPLE || r.width > INT32_MAX / (2 * r.grid) ||
            r.height > INT32_MAX / (2 * r.grid))
            return SR_E_INVALID;
        for (int f = 0; f < 2 * r.n_frames; f++)
            if (r.phases[f] >= r.grid) return SR_E_INVALID;
    }
    if (r.nrows < 0 || r.block_rows <= 0) return SR_E_INVALID;
    if (r.d_codes && (r.n_frames != 1 || r.d_wave_cost)) return SR_E_INVALID;
    if (r.out && r.pitch < (size_t)r.width * 4) return SR_E_INVALID;
    if (r.n_frames > 1 && (!r.out || r.frame_stride < r.pitch * (size_t)r.nrows || r.dbg_rgba || r.dbg_steps))
        return SR_E_INVALID;
    sr_pre::derive_frame({r.cams, r.n_frames, r.params, r.width, r.height, r.grid, r.phases, ctx->cull, ctx->projection,
                          r.phase_cams},
                         seq ? ctx->h_seq[(size_t)r.seq_first] : ctx->h_scene, fr);
    if (seq) {
        // the slot counts pick the integrate kernel's capacity: the window's
        // maxima. The exclusions stay derive_frame's "none": each frame's
        // own are in its start record (ensure_xtab).
        for (int f = 1; f < r.n_frames; f++) {
            const sr_dev_scene& sc = ctx->h_seq[(size_t)(r.seq_first + f)];
            const int cyl = __builtin_popcount((unsigned)sc.budget_cyl_mask);
            if (sc.num_budget > fr.num_budget) fr.num_budget = sc.num_budget;
            if (cyl > fr.num_budget_cyl) fr.num_budget_cyl = cyl;
        }
    }
    context_into_frame(ctx, !seq, fr);
    fr.split_tiles = r.d_codes ? 0 : ctx->split_tiles;
    fr.split_log2 = ctx->split_log2;
    fr.split_min_steps = ctx->split_min_steps;
    fr.fast_unroll = ctx->fast_unroll;
    fr.out_frame_stride = (int64_t)r.frame_stride;
    fr.tiles = ((r.width + 15) / 16) * ((r.nrows + 15) / 16);
    fr.nrows = r.nrows;
    fr.row_base = r.row_base;
    fr.block_rows = r.block_rows;
    fr.block_stride = r.block_stride;
    fr.block_list = r.d_block_list;
    fr.wave_cost = r.d_wave_cost;
    return SR_OK;
}

int launch(sr_ctx* ctx, const Launch& r) {
    sr_dev_frame fr;
    int rc = build_frame(ctx, r, fr);
    if (rc != SR_OK) return rc;
    const hipStream_t s = reinterpret_cast<hipStream_t>(r.stream);
    ctx->kept.valid = false;  // from here on the pixel state is this launch's
    rc = enter_stream(ctx, s);
    if (rc != SR_OK) return rc;
    const float4* tbl = nullptr;
    rc = ensure_table(ctx, r.params->max_steps, r.params->max_revolutions, s, &tbl);
    if (rc != SR_OK) return rc;
    rc = ensure_pixel_state(ctx, (size_t)fr.tiles * (size_t)r.n_frames * 256, s);
    if (rc != SR_OK) return rc;
    if (r.blocks && !fr.block_list) {  // launch_ss and launch_sub_frames resolved theirs
        rc = ensure_block_list(ctx, r.blocks, r.n_blocks, s, &fr.block_list);
        if (rc != SR_OK) return rc;
    }
    int* order[2] = {};  // and the tiles' costs
    if (r.d_codes) {
        order[0] = r.d_codes;  // no cost feedback: order_tiles does not run, last_order stays the plain frame's
    } else if (r.nrows > 0) {
        const int gx = (r.width + 15) / 16, gy = (r.nrows + 15) / 16;
        rc = ensure_order(ctx, gx, gy, fr.block_list, s, order);
        if (rc != SR_OK) return rc;
        ctx->caches.last_order = order[0];
        ctx->caches.last_slots = launch_slots(ctx, (size_t)gx * (size_t)gy);
    }
    const bool seq = r.seq_first != -1;
    const float* xtab = nullptr;
    if (seq) {
        rc = ensure_xtab(ctx, fr.u_f, fr.max_dphi, s, &xtab);
        if (rc != SR_OK) return rc;
    }
    hipEvent_t* const ev4 = ctx->timing_n < ctx->timing_cap ? &ctx->tev[4 * (size_t)ctx->timing_n++] : nullptr;
    const hipError_t e =
        seq ? sr_launch_geodesic_seq(ctx->d_seq + r.seq_first, xtab + (size_t)r.seq_first * kXTabFloats, tbl, ctx->d_segs,
                                     ctx->d_bg, ctx->d_arr, ctx->d_opq, &fr, r.out, r.pitch, r.dbg_rgba, r.dbg_steps,
                                     ctx->d_ps(), ctx->ps_n(), ctx->d_list(), ctx->d_count(), order[0], order[1],
                                     ctx->d_diag, ctx->d_start, ev4, s)
            : sr_launch_geodesic(ctx->d_scene, tbl, ctx->d_segs, ctx->d_bg, ctx->d_arr, ctx->d_opq, &fr, r.out, r.pitch,
                                 r.dbg_rgba, r.dbg_steps, ctx->d_ps(), ctx->ps_n(), ctx->d_list(), ctx->d_count(), order[0],
                                 order[1], ctx->d_diag, ctx->d_start, ev4, s);
    rc = finish(ctx, e, s);
    // the retained frame: whole launches of at least one row (a sparse launch
    // holds only its tiles' rays, sr_wave_costs writes no pixels; the callers
    // that launch more after this one, launch_ss and the rest, amend or drop
    // it). None after a sequence launch: "the current scene" has no meaning for it.
    if (rc == SR_OK && r.nrows > 0 && !r.d_codes && !r.d_wave_cost && !seq) {
        ctx->kept.fr = fr;
        ctx->kept.max_steps = r.params->max_steps;
        ctx->kept.max_revolutions = r.params->max_revolutions;
        ctx->kept.ss = 1;
        ctx->kept.d_blocks = nullptr;
        ctx->kept.valid = true;
    }
    return rc;
}

// The launch `r` into the context's sample scratch (`bytes` of it: rows of `pitch` bytes, frames
// `frame_stride` apart), for a post-kernel of the caller's, which reads the block list's device
// copy too. Every argument was checked by the caller and check_frames.
int launch_into_scratch(sr_ctx* c, Launch& r, size_t bytes, size_t pitch, size_t frame_stride) {
    const hipStream_t s = reinterpret_cast<hipStream_t>(r.stream);
    int rc = enter_stream(c, s);
    if (rc == SR_OK) rc = grow(c, kSs, bytes, 1, s);
    if (rc == SR_OK && r.blocks) rc = ensure_block_list(c, r.blocks, r.n_blocks, s, &r.d_block_list);
    if (rc != SR_OK) return rc;
    return launch(c, r.into(c->d_ss(), pitch, frame_stride));
}

// The sub-frames of a phase launch (sr_render_accumulate, the shutter entry
// points) into the sample scratch, at r.pitch and r.frame_stride. No retained
// frame: the sub-frames are not a caller's output.
int launch_sub_frames(sr_ctx* c, Launch& r) {
    const size_t ipitch = (size_t)r.width * 4, istride = ipitch * (size_t)r.nrows;
    const int rc = launch_into_scratch(c, r, istride * (size_t)r.n_frames, ipitch, istride);
    c->kept.valid = false;
    return rc;
}

// The sub-frames of `r`, then their sum into (reset: over) the caller's accumulator
int accumulate_sub_frames(sr_ctx* c, Launch& r, int reset, uint16_t* accum, size_t accum_pitch) {
    c->kept.valid = false;
    if (r.nrows == 0) return SR_OK;  // no rows: nothing is written
    const int rc = launch_sub_frames(c, r);
    if (rc != SR_OK) return rc;
    // again at the end of the whole: a launch on another stream waits for the add too
    const hipStream_t s = reinterpret_cast<hipStream_t>(r.stream);
    return finish(c, sr_accum_add_device(c->d_ss(), r.pitch, r.frame_stride, r.n_frames, r.width, r.nrows, reset ? 1 : 0,
                                         accum, accum_pitch, s),
                  s);
}

// ---- supersampling: the sample frame is an ordinary launch of the (ss x
// width) x (ss x height) frame into the context's sample scratch, resolved
// to the caller's buffer by resolve.hip on the same stream.
// `o` is the launch in output pixels (one band, or a block list's slots).
int launch_ss(sr_ctx* c, const Launch& o, int ss) {
    if (o.nrows == 0) {  // no rows: nothing is written
        c->kept.valid = false;
        return SR_OK;
    }
    const hipStream_t s = reinterpret_cast<hipStream_t>(o.stream);
    const size_t spitch = (size_t)o.width * 4 * (size_t)ss;
    const size_t sstride = spitch * (size_t)o.nrows * (size_t)ss;
    Launch sample = o;
    sample.width *= ss;
    sample.height *= ss;
    sample.nrows *= ss;
    sample.row_base *= ss;
    sample.block_rows *= ss;
    sample.block_stride *= ss;
    int rc = launch_into_scratch(c, sample, sstride * (size_t)o.n_frames, spitch, o.n_frames > 1 ? sstride : 0);
    if (rc != SR_OK) return rc;
    const hipError_t e = sr_resolve_box_device(c->d_ss(), spitch, sstride, o.width, o.nrows, ss, sample.d_block_list,
                                               o.block_rows, o.height, o.out, o.pitch, o.frame_stride, o.n_frames, s);
    // again at the end of the whole: a launch on another stream waits for the resolve too
    rc = finish(c, e, s);
    if (rc == SR_OK && c->kept.valid) {  // the retained frame is the sample frame and this resolve
        c->kept.ss = ss;
        c->kept.width = o.width;
        c->kept.height = o.height;
        c->kept.rows = o.nrows;
        c->kept.block_rows = o.block_rows;
        c->kept.d_blocks = sample.d_block_list;
    } else {
        c->kept.valid = false;
    }
    return rc;
}

// The shading-only fields of a scene (sr.h "Retained frames") cleared: what is
// left is what hit_opacity_uniform, the step loop and precompute.cpp's
// pack_scene can read.
void clear_shading_fields(sr_scene& s) {
    s.num_lights = 0;
    std::memset(s.lights, 0, sizeof s.lights);
    for (sr_material& m : s.materials) {
        m.color[0] = m.color[1] = m.color[2] = 0.0f;
        m.ambient = m.diffuse = m.specular = m.shininess = 0.0f;
        m.normal_map_index = 0;
    }
}

// sr_reshade and sr_reshade_debug: the retained launch's shade and resume
// kernels again with the context's current scene, background and textures,
// into `o`'s output (its pitch and frame stride) on its stream.
int reshade(sr_ctx* c, const Launch& o) {
    const sr_ctx::Retained& k = c->kept;
    const int n_frames = k.fr.batch;
    const bool ss = k.ss > 1;
    const int width = ss ? k.width : k.fr.width, rows = ss ? k.rows : k.fr.nrows;
    if (o.out && o.pitch < (size_t)width * 4) return SR_E_INVALID;
    if (n_frames > 1 && (!o.out || o.frame_stride < o.pitch * (size_t)rows)) return SR_E_INVALID;
    const hipStream_t s = reinterpret_cast<hipStream_t>(o.stream);
    int rc = enter_stream(c, s);
    if (rc != SR_OK) return rc;
    const float4* tbl = nullptr;
    rc = ensure_table(c, k.max_steps, k.max_revolutions, s, &tbl);
    if (rc != SR_OK) return rc;
    sr_dev_frame fr = k.fr;
    fr.bg_w = c->bg_w;  // sr_set_background keeps the frame: its current image
    fr.bg_h = c->bg_h;
    const size_t spitch = (size_t)k.width * 4 * (size_t)k.ss;
    const size_t sstride = spitch * (size_t)k.rows * (size_t)k.ss;
    if (ss) {
        rc = grow(c, kSs, sstride * (size_t)n_frames, 1, s);
        if (rc != SR_OK) return rc;
        fr.out_frame_stride = (int64_t)(n_frames > 1 ? sstride : 0);
    } else {
        fr.out_frame_stride = (int64_t)o.frame_stride;
    }
    hipError_t e = sr_launch_reshade(c->d_scene, tbl, c->d_segs, c->d_bg, c->d_arr, &fr, ss ? c->d_ss() : o.out,
                                     ss ? spitch : o.pitch, o.dbg_rgba, o.dbg_steps, c->d_ps(), c->ps_n(), c->d_list(),
                                     c->d_count(), c->d_diag, s);
    if (hip_ok(e) && ss)
        e = sr_resolve_box_device(c->d_ss(), spitch, sstride, k.width, k.rows, k.ss, k.d_blocks, k.block_rows, k.height,
                                  o.out, o.pitch, o.frame_stride, n_frames, s);
    return finish(c, e, s);
}

// sr_create's scene image (zeros, no far-field miss radius yet, the default
// test ray), then `s` and `t` where given, as sr_set_scene and sr_set_test_ray
// pack them
int fresh_image(const sr_scene* s, const sr_test_ray* t, sr_dev_scene& d, std::vector<float>& segs) {
    std::memset(&d, 0, sizeof d);
    d.flat_miss_r2 = INFINITY;
    sr_test_ray def;
    sr_test_ray_default(&def);
    int rc = sr_pre::pack_test_ray(def, d, segs);
    if (rc == SR_OK && s) rc = sr_pre::pack_scene(*s, d);
    if (rc == SR_OK && t) rc = sr_pre::pack_test_ray(*t, d, segs);
    return rc;
}

}  // namespace

extern "C" {

int sr_assemble_blocks(const uint8_t* stacked, size_t rank_stride, size_t in_frame_stride, const int* lists,
                       int world, int per, int height, int block_rows, size_t row_bytes, uint8_t* out,
                       size_t out_frame_stride, int n_frames, int on_device, sr_stream stream) {
    if (!stacked || !lists || !out || world <= 0 || per < 0 || height <= 0 || block_rows <= 0 || row_bytes == 0 ||
        n_frames < 1)
        return SR_E_INVALID;
    if (!on_device)
        return sr_assemble_blocks_host(stacked, rank_stride, in_frame_stride, lists, world, per, height, block_rows,
                                       row_bytes, out, out_frame_stride, n_frames);
    return status(sr_assemble_blocks_device(stacked, rank_stride, in_frame_stride, lists, world, per, height,
                                            block_rows, row_bytes, out, out_frame_stride, n_frames,
                                            reinterpret_cast<hipStream_t>(stream)));
}

const char* sr_version(void) { return "schwarzschild-mi355x 0.1 (gfx950)"; }

const char* sr_status_string(int s) {
    switch (s) {
    case SR_OK: return "ok";
    case SR_E_INVALID: return "invalid argument";
    case SR_E_CAPACITY: return "capacity exceeded";
    case SR_E_HIP: return "HIP runtime error";
    case SR_E_NOMEM: return "out of memory";
    case SR_E_NOT_READY: return "scene not set";
    case SR_E_NO_DEVICE: return "no HIP device";
    case SR_E_IO: return "file write failed";
    default: return "unknown status";
    }
}

int sr_create(sr_ctx** out, int hip_device) {
    if (!out) return SR_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (!hip_ok(hipGetDeviceCount(&n)) || n <= 0) return SR_E_NO_DEVICE;
    if (hip_device < 0 || hip_device >= n) return SR_E_NO_DEVICE;
    if (!hip_ok(hipSetDevice(hip_device))) return SR_E_HIP;
    sr_ctx* c = new (std::nothrow) sr_ctx();
    if (!c) return SR_E_NOMEM;
    c->device = hip_device;
    std::memset(&c->h_scene, 0, sizeof c->h_scene);
    c->h_scene.flat_miss_r2 = INFINITY;  // set by sr_set_scene
    if (!hip_ok(hipStreamCreateWithFlags(&c->upload, hipStreamNonBlocking))) {
        c->upload = nullptr;
        sr_destroy(c);
        return SR_E_HIP;
    }
    if (!hip_ok(hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming))) {
        c->order_ev = nullptr;
        sr_destroy(c);
        return SR_E_HIP;
    }
    if (!hip_ok(hipMalloc(&c->d_scene, sizeof(sr_dev_scene))) ||
        !hip_ok(hipMalloc(&c->d_segs, (size_t)SR_SEGS_BUF_FLOATS * sizeof(float))) ||
        !hip_ok(hipMalloc(reinterpret_cast<void**>(&c->d_diag), sizeof(int))) ||
        !hip_ok(hipMalloc(reinterpret_cast<void**>(&c->d_start), SR_MAX_BATCH * sizeof(sr_dev_start)))) {
        sr_destroy(c);
        return SR_E_NOMEM;
    }
    if (!hip_ok(hipMemsetAsync(c->d_scene, 0, sizeof(sr_dev_scene), c->upload)) ||
        !hip_ok(hipMemsetAsync(c->d_diag, 0, sizeof(int), c->upload)) ||
        !hip_ok(hipMemsetAsync(c->d_start, 0, SR_MAX_BATCH * sizeof(sr_dev_start), c->upload)) ||
        !hip_ok(hipMemsetAsync(c->d_segs, 0, (size_t)SR_SEGS_BUF_FLOATS * sizeof(float),
                               c->upload)) ||
        !hip_ok(hipStreamSynchronize(c->upload))) {
        sr_destroy(c);
        return SR_E_HIP;
    }
    sr_test_ray tr;
    sr_test_ray_default(&tr);
    int rc = sr_set_test_ray(c, &tr);
    if (rc != SR_OK) {
        sr_destroy(c);
        return rc;
    }
    *out = c;
    return SR_OK;
}

void sr_destroy(sr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)wait_ctx(c);
    if (c->d_scene) (void)hipFree(c->d_scene);
    if (c->d_segs) (void)hipFree(c->d_segs);
    if (c->d_diag) (void)hipFree(c->d_diag);
    if (c->d_start) (void)hipFree(c->d_start);
    // the rest came from the stream-ordered allocator: freed the same way,
    // then waited for (the context's frames are done: wait_ctx)
    const hipStream_t s = c->upload;
    if (s) {
        c->launched = false;  // release() frees on `s`
        release(c, c->d_bg, s);
        release(c, c->d_arr, s);
        release(c, c->d_opq, s);
        release(c, c->d_seq, s);
        c->caches.release_all(HipDevice{c}, s);
        for (Scratch& b : c->scratch) drop(c, b, s);
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    for (hipEvent_t e : c->tev) (void)hipEventDestroy(e);
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    delete c;
}

int sr_diag_counters(sr_ctx* c, int64_t* out, int n) {
    if (!c || !out || n < 0) return SR_E_INVALID;
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    int dropped = 0;
    if (!hip_ok(hipMemcpyAsync(&dropped, c->d_diag, sizeof(int), hipMemcpyDeviceToHost, c->upload)) ||
        !hip_ok(hipStreamSynchronize(c->upload)))
        return SR_E_HIP;
    const int64_t v[2] = {dropped, c->free_errors};
    for (int i = 0; i < n && i < 2; i++) out[i] = v[i];
    return SR_OK;
}

int sr_set_background(sr_ctx* c, const uint8_t* px, int w, int h, int ch) {
    if (!c || !px || w <= 0 || h <= 0 || (ch != 3 && ch != 4)) return SR_E_INVALID;
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    int rc = upload_rgba(c, px, w, h, 1, ch, &c->d_bg);
    if (rc != SR_OK) {
        c->bg_w = c->bg_h = 0;
        return rc;
    }
    c->bg_w = w;
    c->bg_h = h;
    return SR_OK;
}

int sr_set_texture_array(sr_ctx* c, const uint8_t* px, int w, int h, int layers, int ch) {
    if (!c || !px || w <= 0 || h <= 0 || layers <= 0 || (ch != 3 && ch != 4)) return SR_E_INVALID;
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    c->kept.valid = false;  // the rays' opacity classes read the array (hit_opacity_uniform)
    int rc = upload_rgba(c, px, w, h, layers, ch, &c->d_arr);
    if (rc == SR_OK) {
        const std::vector<uint8_t> bits = sr_pre::opacity_bits(px, w, h, layers, ch);
        rc = upload_bytes(c, bits.data(), bits.size(), reinterpret_cast<void**>(&c->d_opq));
    }
    if (rc != SR_OK) {
        c->arr_w = c->arr_h = c->arr_layers = 0;
        return rc;
    }
    c->arr_w = w;
    c->arr_h = h;
    c->arr_layers = layers;
    return SR_OK;
}

int sr_set_scene(sr_ctx* c, const sr_scene* s) {
    if (!c || !s) return SR_E_INVALID;
    sr_dev_scene d = c->h_scene;  // keeps the test-ray part
    const int rc = sr_pre::pack_scene(*s, d);
    if (rc != SR_OK) return rc;
    // the retained frame outlives a change of shading-only fields alone
    const bool keep = c->scene_set && sr_scene_shading_only(&c->scene_src, s) == 1;
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    if (!keep) c->kept.valid = false;
    if (!hip_ok(hipMemcpyAsync(c->d_scene, &d, sizeof d, hipMemcpyHostToDevice, c->upload)) ||
        !hip_ok(hipStreamSynchronize(c->upload))) {
        c->kept.valid = false;
        return SR_E_HIP;
    }
    c->h_scene = d;
    c->scene_src = *s;
    c->xc_uf = c->xc_dphi = NAN;  // the low-energy exclusions again at the next launch
    c->scene_set = true;
    return SR_OK;
}

int sr_set_test_ray(sr_ctx* c, const sr_test_ray* t) {
    if (!c || !t) return SR_E_INVALID;
    sr_dev_scene d = c->h_scene;  // keeps the scene part
    std::vector<float> segs;
    const int rc = sr_pre::pack_test_ray(*t, d, segs);
    if (rc != SR_OK) return rc;
    c->kept.valid = false;  // the test ray is geometry of the retained rays
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    if (!hip_ok(hipMemcpyAsync(c->d_segs, segs.data(), segs.size() * sizeof(float), hipMemcpyHostToDevice,
                               c->upload)) ||
        !hip_ok(hipMemcpyAsync(c->d_scene, &d, sizeof d, hipMemcpyHostToDevice, c->upload)) ||
        !hip_ok(hipStreamSynchronize(c->upload)))
        return SR_E_HIP;
    c->h_scene = d;
    // the sequence's scenes carry the test-ray part too (it passed above:
    // pack_test_ray rejects ahead of any write, and not by the scene part)
    if (!c->h_seq.empty()) {
        for (sr_dev_scene& q : c->h_seq) (void)sr_pre::pack_test_ray(*t, q, segs);
        if (!hip_ok(hipMemcpyAsync(c->d_seq, c->h_seq.data(), c->h_seq.size() * sizeof(sr_dev_scene),
                                   hipMemcpyHostToDevice, c->upload)) ||
            !hip_ok(hipStreamSynchronize(c->upload)))
            return SR_E_HIP;
    }
    return SR_OK;
}

// ---- scene sequences (sr.h): the scenes of an animation as one device
// array; a launch renders frame f from scene first_scene + f (Launch::sequence)

int sr_set_scene_sequence(sr_ctx* c, const sr_scene* scenes, int n) {
    if (!c || n < 0 || (n > 0 && !scenes)) return SR_E_INVALID;
    if (n > SR_MAX_SEQUENCE) return SR_E_CAPACITY;
    std::vector<sr_dev_scene> seq((size_t)n, c->h_scene);  // the context's test-ray part (sr_set_scene's own start)
    for (int k = 0; k < n; k++) {
        const int rc = sr_pre::pack_scene(scenes[k], seq[(size_t)k]);
        if (rc != SR_OK) return rc;  // the earlier sequence stays
    }
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    // the tables of the sequence that goes (the frames are done, the frees stream-ordered all the same)
    c->caches.xtabs.release_all(HipDevice{c}, c->upload);
    c->h_seq.clear();
    if (n == 0) {
        release(c, c->d_seq, c->upload);
        c->d_seq = nullptr;
        return SR_OK;
    }
    const int rc = upload_bytes(c, seq.data(), seq.size() * sizeof(sr_dev_scene), reinterpret_cast<void**>(&c->d_seq));
    if (rc != SR_OK) {
        release(c, c->d_seq, c->upload);
        c->d_seq = nullptr;
        return rc;
    }
    c->h_seq = std::move(seq);
    return SR_OK;
}

int sr_scene_sequence_length(sr_ctx* c) { return c ? (int)c->h_seq.size() : SR_E_INVALID; }

int sr_render(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int row_begin,
              int row_end, uint8_t* out, size_t pitch, sr_stream stream) {
    if (!out || bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    return launch(c, Launch(cam, 1, p, width, height, stream).band(row_begin, row_end - row_begin).into(out, pitch));
}

int sr_blocks_row_count(int height, int block_rows, int block_first, int block_step) {
    if (height <= 0 || block_rows <= 0 || block_first < 0 || block_step <= 0) return 0;
    int rows = 0;
    for (int b = block_first; b * block_rows < height; b += block_step) {
        int r = height - b * block_rows;
        rows += r < block_rows ? r : block_rows;
    }
    return rows;
}

int sr_render_blocks(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int block_rows,
                     int block_first, int block_step, uint8_t* out, size_t pitch, sr_stream stream) {
    return sr_render_blocks_batch(c, cam, 1, p, width, height, block_rows, block_first, block_step, out, pitch, 0,
                                  stream);
}

int sr_wave_costs(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int32_t* dev_out,
                  sr_stream stream) {
    if (!c || !cam || !dev_out || width <= 0 || height <= 0) return SR_E_INVALID;
    Launch r = Launch(cam, 1, p, width, height, stream).band(0, height).into(nullptr, (size_t)width * 4);
    r.block_stride = height;
    r.d_wave_cost = dev_out;
    // split tiles off for this launch: every wave is a whole 8x8 wave tile
    const int split = c->split_tiles;
    c->split_tiles = 0;
    const int rc = launch(c, r);
    c->split_tiles = split;
    return rc;
}

int sr_render_block_list(sr_ctx* c, const sr_camera* cams, int n_frames, const sr_params* p, int width, int height,
                         int block_rows, const int* blocks, int n_blocks, uint8_t* out, size_t pitch,
                         size_t frame_stride, sr_stream stream) {
    const int rc = check_block_list(c, out, blocks, n_blocks, block_rows, height, 1);
    if (rc != SR_OK) return rc;
    return launch(c, Launch(cams, n_frames, p, width, height, stream)
                         .block_list(blocks, n_blocks, block_rows)
                         .into(out, pitch, frame_stride));
}

int sr_render_blocks_batch(sr_ctx* c, const sr_camera* cams, int n_frames, const sr_params* p, int width,
                           int height, int block_rows, int block_first, int block_step, uint8_t* out, size_t pitch,
                           size_t frame_stride, sr_stream stream) {
    if (!out || block_rows <= 0 || block_first < 0 || block_step <= 0) return SR_E_INVALID;
    return launch(c, Launch(cams, n_frames, p, width, height, stream)
                         .strided_blocks(block_rows, block_first, block_step)
                         .into(out, pitch, frame_stride));
}

static bool bad_grid(int ss) { return ss < 1 || ss > SR_MAX_SUPERSAMPLE; }

// The bounds of a supersampled launch's output (`rows` of it; a block list's: bounded by
// check_block_list already): the sample frame's sizes fit an int, its rows 2^24; then the frame stride's
static int check_ss_output(int width, int height, int rows, int ss, int n_frames, size_t pitch, size_t frame_stride) {
    if (pitch < (size_t)width * 4 || width > INT32_MAX / (4 * ss) || height > INT32_MAX / ss || rows > (1 << 24) / ss)
        return SR_E_INVALID;
    return n_frames > 1 && frame_stride < pitch * (size_t)rows ? SR_E_INVALID : SR_OK;
}

int sr_render_sequence(sr_ctx* c, int first_scene, const sr_camera* cams, int n_frames, const sr_params* p, int width,
                       int height, int row_begin, int row_end, int ss, uint8_t* out, size_t pitch,
                       size_t frame_stride, sr_stream stream) {
    if (bad_grid(ss)) return SR_E_INVALID;
    if (!out || bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    const int n = row_end - row_begin;
    const Launch r = Launch(cams, n_frames, p, width, height, stream)
                         .band(row_begin, n)
                         .sequence(first_scene)
                         .into(out, pitch, frame_stride);
    if (ss == 1) return launch(c, r);
    int rc = check_frames(c, cams, n_frames, p, width, height, r.seq_first);
    if (rc == SR_OK) rc = check_ss_output(width, height, n, ss, n_frames, pitch, frame_stride);
    if (rc != SR_OK) return rc;
    return launch_ss(c, r, ss);
}

int sr_render_sequence_block_list(sr_ctx* c, int first_scene, const sr_camera* cams, int n_frames, const sr_params* p,
                                  int width, int height, int block_rows, const int* blocks, int n_blocks, int ss,
                                  uint8_t* out, size_t pitch, size_t frame_stride, sr_stream stream) {
    if (bad_grid(ss)) return SR_E_INVALID;
    int rc = check_block_list(c, out, blocks, n_blocks, block_rows, height, ss);
    if (rc == SR_OK) rc = check_frames(c, cams, n_frames, p, width, height, first_scene < 0 ? INT32_MIN : first_scene);
    if (rc == SR_OK) rc = check_ss_output(width, height, n_blocks * block_rows, ss, n_frames, pitch, frame_stride);
    if (rc != SR_OK) return rc;
    const Launch r = Launch(cams, n_frames, p, width, height, stream)
                         .block_list(blocks, n_blocks, block_rows)
                         .sequence(first_scene)
                         .into(out, pitch, frame_stride);
    return ss == 1 ? launch(c, r) : launch_ss(c, r, ss);
}

int sr_render_sequence_debug(sr_ctx* c, int scene_index, const sr_camera* cam, const sr_params* p, int width,
                             int height, int row_begin, int row_end, float* dbg_rgba, uint8_t* out,
                             int32_t* dbg_steps, sr_stream stream) {
    if (bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    if (!dbg_rgba && !out && !dbg_steps) return SR_E_INVALID;
    Launch r = Launch(cam, 1, p, width, height, stream)
                   .band(row_begin, row_end - row_begin)
                   .sequence(scene_index)
                   .into(out, (size_t)width * 4);
    r.dbg_rgba = dbg_rgba;
    r.dbg_steps = dbg_steps;
    return launch(c, r);
}

int sr_resolve_box(const uint8_t* samples, size_t sample_pitch, size_t sample_frame_stride, int width, int rows, int ss,
                   uint8_t* out, size_t pitch, size_t out_frame_stride, int n_frames, int on_device,
                   sr_stream stream) {
    if (ss < 1 || ss > SR_MAX_SUPERSAMPLE) return SR_E_INVALID;
    if (!samples || !out || width <= 0 || rows < 0 || n_frames < 1) return SR_E_INVALID;
    if (width > INT32_MAX / (4 * ss) || rows > (1 << 24) / ss) return SR_E_INVALID;
    if (pitch < (size_t)width * 4 || sample_pitch < (size_t)width * 4 * (size_t)ss) return SR_E_INVALID;
    if (n_frames > 1 &&
        (out_frame_stride < pitch * (size_t)rows || sample_frame_stride < sample_pitch * (size_t)rows * (size_t)ss))
        return SR_E_INVALID;
    if (!on_device)
        return sr_resolve_box_host(samples, sample_pitch, sample_frame_stride, width, rows, ss, out, pitch,
                                   out_frame_stride, n_frames),
               SR_OK;
    return status(sr_resolve_box_device(samples, sample_pitch, sample_frame_stride, width, rows, ss, nullptr, 0, rows,
                                        out, pitch, out_frame_stride, n_frames, reinterpret_cast<hipStream_t>(stream)));
}

int sr_render_ss(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int row_begin,
                 int row_end, int ss, uint8_t* out, size_t pitch, sr_stream stream) {
    if (bad_grid(ss)) return SR_E_INVALID;
    if (ss == 1) return sr_render(c, cam, p, width, height, row_begin, row_end, out, pitch, stream);
    if (!out || bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    const int n = row_end - row_begin;
    int rc = check_frames(c, cam, 1, p, width, height);
    if (rc == SR_OK) rc = check_ss_output(width, height, n, ss, 1, pitch, 0);
    if (rc != SR_OK) return rc;
    return launch_ss(c, Launch(cam, 1, p, width, height, stream).band(row_begin, n).into(out, pitch), ss);
}

int sr_render_block_list_ss(sr_ctx* c, const sr_camera* cams, int n_frames, const sr_params* p, int width,
                            int height, int block_rows, const int* blocks, int n_blocks, int ss, uint8_t* out,
                            size_t pitch, size_t frame_stride, sr_stream stream) {
    if (bad_grid(ss)) return SR_E_INVALID;
    if (ss == 1)
        return sr_render_block_list(c, cams, n_frames, p, width, height, block_rows, blocks, n_blocks, out, pitch,
                                    frame_stride, stream);
    int rc = check_block_list(c, out, blocks, n_blocks, block_rows, height, ss);
    if (rc == SR_OK) rc = check_frames(c, cams, n_frames, p, width, height);
    if (rc == SR_OK) rc = check_ss_output(width, height, n_blocks * block_rows, ss, n_frames, pitch, frame_stride);
    if (rc != SR_OK) return rc;
    return launch_ss(c, Launch(cams, n_frames, p, width, height, stream)
                            .block_list(blocks, n_blocks, block_rows)
                            .into(out, pitch, frame_stride),
                     ss);
}

// ---- sample phases: a launch of the output frame's own shape (grid, pixel
// state, launch order) whose pixels are one sub-sample position of the sample
// frame (Launch::phases), and the 16-bit accumulator that sums them
// (accum.hip)

int sr_render_phase(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int row_begin,
                    int row_end, int ss, int phase_x, int phase_y, uint8_t* out, size_t pitch, sr_stream stream) {
    if (bad_grid(ss) || phase_x < 0 || phase_x >= ss || phase_y < 0 || phase_y >= ss) return SR_E_INVALID;
    if (!out || bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    const uint8_t phase[2] = {(uint8_t)phase_x, (uint8_t)phase_y};
    Launch r = Launch(cam, 1, p, width, height, stream).band(row_begin, row_end - row_begin).into(out, pitch);
    r.grid = ss;
    r.phases = phase;
    return launch(c, r);
}

int sr_render_accumulate(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int row_begin,
                         int row_end, int ss, const uint8_t* phases, int n_phases, int reset, uint16_t* accum,
                         size_t accum_pitch, sr_stream stream) {
    if (bad_grid(ss) || !phases || !accum || n_phases < 1) return SR_E_INVALID;
    if (n_phases > SR_MAX_BATCH) return SR_E_CAPACITY;
    for (int f = 0; f < 2 * n_phases; f++)
        if (phases[f] >= ss) return SR_E_INVALID;
    if (bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    int rc = check_frames(c, cam, 1, p, width, height);
    if (rc != SR_OK) return rc;
    if (width > INT32_MAX / 8 || accum_pitch < (size_t)width * 8 || (((uintptr_t)accum | accum_pitch) & 7) != 0)
        return SR_E_INVALID;
    Launch r = Launch(cam, n_phases, p, width, height, stream).band(row_begin, row_end - row_begin);
    r.grid = ss;
    r.phases = phases;
    return accumulate_sub_frames(c, r, reset, accum, accum_pitch);
}

int sr_accum_add(const uint8_t* images, size_t pitch, size_t image_stride, int n_images, int width, int rows, int reset,
                 uint16_t* accum, size_t accum_pitch, int on_device, sr_stream stream) {
    if (!images || !accum || width <= 0 || rows < 0 || n_images < 1 || n_images > SR_MAX_ACCUM_PASSES)
        return SR_E_INVALID;
    if (width > INT32_MAX / 8 || pitch < (size_t)width * 4 || accum_pitch < (size_t)width * 8) return SR_E_INVALID;
    if (n_images > 1 && image_stride < pitch * (size_t)rows) return SR_E_INVALID;
    if ((((uintptr_t)images | pitch | (n_images > 1 ? image_stride : 0)) & 3) != 0) return SR_E_INVALID;
    if ((((uintptr_t)accum | accum_pitch) & 7) != 0) return SR_E_INVALID;
    if (!on_device)
        return sr_accum_add_host(images, pitch, image_stride, n_images, width, rows, reset ? 1 : 0, accum, accum_pitch),
               SR_OK;
    return status(sr_accum_add_device(images, pitch, image_stride, n_images, width, rows, reset ? 1 : 0, accum,
                                      accum_pitch, reinterpret_cast<hipStream_t>(stream)));
}

int sr_accum_resolve(const uint16_t* accum, size_t accum_pitch, int width, int rows, int n, uint8_t* out, size_t pitch,
                     int on_device, sr_stream stream) {
    if (!accum || !out || width <= 0 || rows < 0 || n < 1 || n > SR_MAX_ACCUM_PASSES) return SR_E_INVALID;
    if (width > INT32_MAX / 8 || pitch < (size_t)width * 4 || accum_pitch < (size_t)width * 8) return SR_E_INVALID;
    if ((((uintptr_t)accum | accum_pitch) & 7) != 0 || (((uintptr_t)out | pitch) & 3) != 0) return SR_E_INVALID;
    if (!on_device) return sr_accum_resolve_host(accum, accum_pitch, width, rows, n, out, pitch), SR_OK;
    return status(sr_accum_resolve_device(accum, accum_pitch, width, rows, n, out, pitch,
                                          reinterpret_cast<hipStream_t>(stream)));
}

int sr_phase_order(int ss, int k, int* phase_x, int* phase_y) {
    // ss 2, 4: the 2x2 and 4x4 ordered-dither matrices read by rank; ss 3:
    // the centre, the diagonal, the other corners, then the edge midpoints
    static const uint8_t order1[1][2] = {{0, 0}};
    static const uint8_t order2[4][2] = {{0, 0}, {1, 1}, {1, 0}, {0, 1}};
    static const uint8_t order3[9][2] = {{1, 1}, {0, 0}, {2, 2}, {2, 0}, {0, 2}, {1, 0}, {1, 2}, {0, 1}, {2, 1}};
    static const uint8_t order4[16][2] = {{0, 0}, {2, 2}, {2, 0}, {0, 2}, {1, 1}, {3, 3}, {3, 1}, {1, 3},
                                          {1, 0}, {3, 2}, {3, 0}, {1, 2}, {0, 1}, {2, 3}, {2, 1}, {0, 3}};
    static const uint8_t(*const orders[4])[2] = {order1, order2, order3, order4};
    if (bad_grid(ss) || k < 0 || k >= ss * ss || !phase_x || !phase_y) return SR_E_INVALID;
    *phase_x = orders[ss - 1][k][0];
    *phase_y = orders[ss - 1][k][1];
    return SR_OK;
}

// ---- shutter frames (sr.h): the sub-frames are ONE phase launch whose frames
// carry their own cameras and, under a sequence, their own scenes
// (Launch::phase_cams) into the context's sample scratch; shutter.hip resolves
// each group of sub_frames images to its output frame, or accum.hip adds them
// to the caller's accumulator, on the same stream

int sr_shutter_phases(int ss, int sub_frames, uint8_t* out_pairs) {
    if (bad_grid(ss) || sub_frames < 1 || !out_pairs) return SR_E_INVALID;
    for (int k = 0; k < sub_frames; k++) {
        int x = 0, y = 0;
        (void)sr_phase_order(ss, k % (ss * ss), &x, &y);
        out_pairs[2 * k] = (uint8_t)x;
        out_pairs[2 * k + 1] = (uint8_t)y;
    }
    return SR_OK;
}

}  // extern "C"

namespace {

// The sub-frame launch of the three shutter entry points: `groups` groups of
// `sub` frames each (the accumulate form: one group), the caller's phases or
// the default ones in `pairs`
struct ShutterLaunch {
    Launch r;
    uint8_t pairs[2 * SR_MAX_BATCH];
};

// Every rejection of the sub-frames ahead of any allocation, and their launch
// without its rows and output. (the status, then `out` on SR_OK)
int shutter_frames(const sr_ctx* c, int first_scene, const sr_camera* cams, const uint8_t* phases, int sub, int groups,
                   const sr_params* p, int width, int height, int ss, sr_stream stream, ShutterLaunch& out) {
    if (!c || !cams || sub < 1 || groups < 1 || bad_grid(ss) || first_scene < SR_SHUTTER_OWN_SCENE) return SR_E_INVALID;
    if ((long long)sub * groups > SR_MAX_BATCH) return SR_E_CAPACITY;
    const int n = sub * groups;
    if (phases) {
        for (int f = 0; f < 2 * n; f++)
            if (phases[f] >= ss) return SR_E_INVALID;
        std::memcpy(out.pairs, phases, 2 * (size_t)n);
    } else {
        (void)sr_shutter_phases(ss, sub, out.pairs);
        for (int g = 1; g < groups; g++) std::memcpy(out.pairs + 2 * (size_t)g * sub, out.pairs, 2 * (size_t)sub);
    }
    const bool own = first_scene == SR_SHUTTER_OWN_SCENE;
    const int rc = check_frames(c, cams, n, p, width, height, own ? -1 : first_scene);
    if (rc != SR_OK) return rc;
    // build_frame's bounds of a phase launch
    if (width > INT32_MAX / (4 * ss) || height > INT32_MAX / (2 * ss)) return SR_E_INVALID;
    out.r = Launch(cams, n, p, width, height, stream);
    out.r.grid = ss;
    out.r.phases = out.pairs;
    out.r.phase_cams = true;
    if (!own) out.r.sequence(first_scene);
    return SR_OK;
}

// The sub-frames (rows and block list set in sl.r), then their resolve to
// `groups` frames at `out`
int launch_shutter(sr_ctx* c, ShutterLaunch& sl, int sub, int groups, uint8_t* out, size_t pitch, size_t frame_stride) {
    Launch& r = sl.r;
    c->kept.valid = false;
    if (r.nrows == 0) return SR_OK;  // no rows: nothing is written
    const int rc = launch_sub_frames(c, r);
    if (rc != SR_OK) return rc;
    // again at the end of the whole: a launch on another stream waits for the resolve too
    const hipStream_t s = reinterpret_cast<hipStream_t>(r.stream);
    return finish(c, sr_shutter_resolve_device(c->d_ss(), r.pitch, r.frame_stride, sub, groups, r.width, r.nrows,
                                               r.d_block_list, r.block_rows, r.height, out, pitch,
                                               groups > 1 ? frame_stride : 0, s),
                  s);
}

}  // namespace

extern "C" {

int sr_render_shutter(sr_ctx* c, int first_scene, const sr_camera* cams, const uint8_t* phases, int sub_frames,
                      int n_frames, const sr_params* p, int width, int height, int row_begin, int row_end, int ss,
                      uint8_t* out, size_t pitch, size_t frame_stride, sr_stream stream) {
    if (!out || bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    ShutterLaunch sl;
    const int rc = shutter_frames(c, first_scene, cams, phases, sub_frames, n_frames, p, width, height, ss, stream, sl);
    if (rc != SR_OK) return rc;
    const int n = row_end - row_begin;
    if (pitch < (size_t)width * 4 || n > (1 << 24) || (((uintptr_t)out | pitch) & 3) != 0) return SR_E_INVALID;
    if (n_frames > 1 && (frame_stride < pitch * (size_t)n || (frame_stride & 3) != 0)) return SR_E_INVALID;
    sl.r.band(row_begin, n);
    return launch_shutter(c, sl, sub_frames, n_frames, out, pitch, frame_stride);
}

int sr_render_shutter_block_list(sr_ctx* c, int first_scene, const sr_camera* cams, const uint8_t* phases,
                                 int sub_frames, int n_frames, const sr_params* p, int width, int height,
                                 int block_rows, const int* blocks, int n_blocks, int ss, uint8_t* out, size_t pitch,
                                 size_t frame_stride, sr_stream stream) {
    int rc = check_block_list(c, out, blocks, n_blocks, block_rows, height, 1);
    if (rc != SR_OK) return rc;
    ShutterLaunch sl;
    rc = shutter_frames(c, first_scene, cams, phases, sub_frames, n_frames, p, width, height, ss, stream, sl);
    if (rc != SR_OK) return rc;
    if (pitch < (size_t)width * 4 || (((uintptr_t)out | pitch) & 3) != 0) return SR_E_INVALID;
    if (n_frames > 1 && (frame_stride < pitch * (size_t)(n_blocks * block_rows) || (frame_stride & 3) != 0))
        return SR_E_INVALID;
    sl.r.block_list(blocks, n_blocks, block_rows);
    return launch_shutter(c, sl, sub_frames, n_frames, out, pitch, frame_stride);
}

int sr_render_accumulate_shutter(sr_ctx* c, int first_scene, const sr_camera* cams, const uint8_t* phases, int n_sub,
                                 const sr_params* p, int width, int height, int row_begin, int row_end, int ss, int reset,
                                 uint16_t* accum, size_t accum_pitch, sr_stream stream) {
    if (!accum || bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    ShutterLaunch sl;
    int rc = shutter_frames(c, first_scene, cams, phases, n_sub, 1, p, width, height, ss, stream, sl);
    if (rc != SR_OK) return rc;
    if (width > INT32_MAX / 8 || accum_pitch < (size_t)width * 8 || (((uintptr_t)accum | accum_pitch) & 7) != 0)
        return SR_E_INVALID;
    const int n = row_end - row_begin;
    if (n > (1 << 24)) return SR_E_INVALID;
    return accumulate_sub_frames(c, sl.r.band(row_begin, n), reset, accum, accum_pitch);
}

int sr_shutter_resolve(const uint8_t* images, size_t pitch, size_t image_stride, int sub_frames, int n_frames, int width,
                       int rows, uint8_t* out, size_t out_pitch, size_t out_frame_stride, int on_device,
                       sr_stream stream) {
    if (!images || !out || width <= 0 || rows < 0 || sub_frames < 1 || sub_frames > SR_MAX_ACCUM_PASSES || n_frames < 1 ||
        n_frames > 65535)
        return SR_E_INVALID;
    if (width > INT32_MAX / 4 || rows > (1 << 24) || pitch < (size_t)width * 4 || out_pitch < (size_t)width * 4)
        return SR_E_INVALID;
    const bool many = sub_frames > 1 || n_frames > 1;
    if (many && image_stride < pitch * (size_t)rows) return SR_E_INVALID;
    if (n_frames > 1 && out_frame_stride < out_pitch * (size_t)rows) return SR_E_INVALID;
    if ((((uintptr_t)images | pitch | (many ? image_stride : 0)) & 3) != 0) return SR_E_INVALID;
    if ((((uintptr_t)out | out_pitch | (n_frames > 1 ? out_frame_stride : 0)) & 3) != 0) return SR_E_INVALID;
    if (!on_device)
        return sr_shutter_resolve_host(images, pitch, image_stride, sub_frames, n_frames, width, rows, out, out_pitch,
                                       out_frame_stride),
               SR_OK;
    // a stride nothing is read at does not pick the path
    return status(sr_shutter_resolve_device(images, pitch, many ? image_stride : 0, sub_frames, n_frames, width, rows,
                                            nullptr, 0, rows, out, out_pitch, n_frames > 1 ? out_frame_stride : 0,
                                            reinterpret_cast<hipStream_t>(stream)));
}

// ---- adaptive supersampling: the plain frame P into the caller's buffer,
// the selection of its edge tiles (adaptive.hip), a sparse launch of the
// sample frame for the flagged tiles only, and their masked resolve over P,
// all on the caller's stream with no host wait

int sr_edge_tiles(const uint8_t* rgba8, size_t pitch, int width, int height, int threshold, int grow,
                  uint8_t* tile_mask, int on_device, sr_stream stream) {
    if (!rgba8 || !tile_mask || width <= 0 || height <= 0 || grow < 0 || grow > 2) return SR_E_INVALID;
    if (pitch < (size_t)width * 4) return SR_E_INVALID;
    if ((long long)((width + 15) / 16) * ((height + 15) / 16) > INT32_MAX) return SR_E_INVALID;
    if (!on_device) return sr_edge_tiles_host(rgba8, pitch, width, height, threshold, grow, tile_mask), SR_OK;
    return status(sr_edge_tiles_device(rgba8, pitch, width, height, threshold, grow, tile_mask,
                                       reinterpret_cast<hipStream_t>(stream)));
}

int sr_render_adaptive(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int ss,
                       int threshold, int grow_tiles, uint8_t* out, size_t pitch, uint8_t* dev_tile_mask,
                       sr_stream stream) {
    if (ss < 2 || ss > SR_MAX_SUPERSAMPLE || grow_tiles < 0 || grow_tiles > 2 || !out) return SR_E_INVALID;
    int rc = check_frames(c, cam, 1, p, width, height);
    if (rc != SR_OK) return rc;
    if (pitch < (size_t)width * 4 || width > INT32_MAX / (4 * ss) || height > (1 << 24) / ss) return SR_E_INVALID;
    const size_t tiles = (size_t)((width + 15) / 16) * (size_t)((height + 15) / 16);
    const size_t stiles = (size_t)((ss * width + 15) / 16) * (size_t)((ss * height + 15) / 16);
    if (stiles > ((size_t)1 << 22)) return SR_E_INVALID;  // a launch code is tile << 8 in an int
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // P: the whole plain frame, an ordinary launch
    const Launch plain = Launch(cam, 1, p, width, height, stream).band(0, height).into(out, pitch);
    if (threshold >= 255) {  // no tile can be flagged: the plain frame, no sample work
        rc = launch(c, plain);
        c->kept.valid = false;  // no retained frame after an adaptive call, whatever it launched
        if (rc != SR_OK || !dev_tile_mask) return rc;
        return finish(c, hipMemsetAsync(dev_tile_mask, 0, tiles, s), s);
    }
    rc = enter_stream(c, s);
    if (rc != SR_OK) return rc;
    // every buffer of the call ahead of its first launch: SR_E_NOMEM with
    // nothing launched. The pixel state is the whole sample frame's (the
    // integrate kernel's ids are the frame's), which holds the plain frame's.
    const size_t spitch = (size_t)width * 4 * (size_t)ss;
    rc = grow(c, kSs, spitch * (size_t)height * (size_t)ss, 1, s);
    if (rc == SR_OK) rc = grow(c, kAmask, tiles, 1, s);
    if (rc == SR_OK) rc = grow(c, kAcodes, stiles, sizeof(int), s);
    if (rc == SR_OK) rc = ensure_pixel_state(c, stiles * 256, s);
    if (rc != SR_OK) return rc;
    rc = launch(c, plain);  // runs and learns the plain frame's order
    c->kept.valid = false;  // the sparse sample launch below overwrites P's rays
    if (rc != SR_OK) return rc;
    hipError_t e = sr_edge_tiles_device(out, pitch, width, height, threshold, grow_tiles, c->d_amask(), s);
    // the sample tiles in the order P's launch just learned (its shade kernel wrote it): costliest first
    const sr_cache::Caches& cc = c->caches;
    if (hip_ok(e) && (!cc.last_order || cc.last_slots > (size_t)INT32_MAX)) e = hipErrorInvalidValue;
    if (hip_ok(e))
        e = sr_adaptive_codes_device(c->d_amask(), width, height, ss, cc.last_order, (int)cc.last_slots, c->d_acodes(),
                                     dev_tile_mask, s);
    if (!hip_ok(e)) return SR_E_HIP;
    // S, the flagged tiles' part of it
    Launch sample = Launch(cam, 1, p, ss * width, ss * height, stream).band(0, ss * height).into(c->d_ss(), spitch);
    sample.d_codes = c->d_acodes();
    rc = launch(c, sample);
    if (rc != SR_OK) return rc;
    // again at the end of the whole: a launch on another stream waits for the resolve too
    return finish(c, sr_resolve_box_masked_device(c->d_ss(), spitch, width, height, ss, c->d_amask(), out, pitch, s), s);
}

int sr_render_debug(sr_ctx* c, const sr_camera* cam, const sr_params* p, int width, int height, int row_begin,
                    int row_end, float* dbg_rgba, uint8_t* out, int32_t* dbg_steps, sr_stream stream) {
    if (bad_rows(row_begin, row_end, height)) return SR_E_INVALID;
    if (!dbg_rgba && !out && !dbg_steps) return SR_E_INVALID;
    Launch r = Launch(cam, 1, p, width, height, stream)
                   .band(row_begin, row_end - row_begin)
                   .into(out, (size_t)width * 4);
    r.dbg_rgba = dbg_rgba;
    r.dbg_steps = dbg_steps;
    return launch(c, r);
}

// ---- retained frames (sr.h): the pixel state of the context's last launch,
// shaded again (sr_reshade) or read for its first surfaces (sr_pick_map)

int sr_scene_shading_only(const sr_scene* a, const sr_scene* b) {
    if (!a || !b) return 0;
    sr_scene x = *a, y = *b;
    clear_shading_fields(x);
    clear_shading_fields(y);
    return std::memcmp(&x, &y, sizeof x) == 0 ? 1 : 0;  // bytes: a NaN equals itself
}

int sr_can_reshade(sr_ctx* c) { return c && c->scene_set && c->kept.valid ? 1 : 0; }

int sr_reshade(sr_ctx* c, uint8_t* out, size_t pitch, size_t frame_stride, sr_stream stream) {
    if (!c) return SR_E_INVALID;
    if (!sr_can_reshade(c)) return SR_E_NOT_READY;
    if (!out) return SR_E_INVALID;
    Launch o;
    o.stream = stream;
    return reshade(c, o.into(out, pitch, frame_stride));
}

int sr_reshade_debug(sr_ctx* c, float* dbg_rgba, uint8_t* out, int32_t* dbg_steps, sr_stream stream) {
    if (!c) return SR_E_INVALID;
    if (!sr_can_reshade(c)) return SR_E_NOT_READY;
    if (c->kept.fr.batch != 1 || c->kept.ss > 1) return SR_E_INVALID;
    if (!dbg_rgba && !out && !dbg_steps) return SR_E_INVALID;
    Launch o;
    o.stream = stream;
    o.dbg_rgba = dbg_rgba;
    o.dbg_steps = dbg_steps;
    return reshade(c, o.into(out, (size_t)c->kept.fr.width * 4));
}

int sr_pick_map(sr_ctx* c, int32_t* ids, size_t pitch, size_t frame_stride, sr_stream stream) {
    if (!c) return SR_E_INVALID;
    if (!sr_can_reshade(c) || c->kept.ss > 1) return SR_E_NOT_READY;
    const sr_dev_frame& fr = c->kept.fr;
    if (!ids || ((uintptr_t)ids & 3) != 0 || (pitch & 3) != 0 || pitch < (size_t)fr.width * 4) return SR_E_INVALID;
    if (fr.batch > 1 && ((frame_stride & 3) != 0 || frame_stride < pitch * (size_t)fr.nrows)) return SR_E_INVALID;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = enter_stream(c, s);
    if (rc != SR_OK) return rc;
    return finish(c, sr_launch_pick(c->d_scene, c->d_segs, &fr, c->d_ps(), c->ps_n(), ids, pitch,
                                    fr.batch > 1 ? frame_stride : 0, s),
                  s);
}

// ---- ray maps (sr.h): the lens map and the first surface's G-buffer of the
// retained frame. The worklist of the pixels to walk on is the context's own
// resume queue (d_list, d_count: grown with the pixel state, released by
// sr_destroy), free between the context's ordered launches.

int sr_ray_maps(sr_ctx* c, const sr_ray_map_ptrs* m, size_t pitch, size_t frame_stride, sr_stream stream) {
    if (!c || !m) return SR_E_INVALID;
    if (!sr_can_reshade(c) || c->kept.ss > 1) return SR_E_NOT_READY;
    const sr_ctx::Retained& k = c->kept;
    const void* const ptrs[9] = {m->end,        m->id,       m->sky_dir,  m->sky_uv,  m->hit_point,
                                 m->hit_normal, m->hit_view, m->hit_base, m->hit_step};
    bool any = false;
    for (const void* q : ptrs) {
        if (((uintptr_t)q & 3) != 0) return SR_E_INVALID;
        any = any || q != nullptr;
    }
    if (!any || pitch < (size_t)k.fr.width) return SR_E_INVALID;
    if (k.fr.batch > 1 && frame_stride < pitch * (size_t)k.fr.nrows) return SR_E_INVALID;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = enter_stream(c, s);
    if (rc != SR_OK) return rc;
    const float4* tbl = nullptr;  // the step table of the retained schedule, for the pixels walked on
    rc = ensure_table(c, k.max_steps, k.max_revolutions, s, &tbl);
    if (rc != SR_OK) return rc;
    return finish(c, sr_launch_ray_maps(c->d_scene, tbl, c->d_segs, c->d_arr, &k.fr, c->d_ps(), c->ps_n(), m, pitch,
                                        k.fr.batch > 1 ? frame_stride : 0, c->d_list(), c->d_count(), s),
                  s);
}

namespace {
struct HostAtan2 {
    float operator()(float y, float x) const { return (float)std::atan2((double)y, (double)x); }
};
struct HostAsin {
    float operator()(float x) const { return (float)std::asin((double)x); }
};
}  // namespace

int sr_sky_uv(const float dir[3], float out_uv[2]) {
    if (!dir || !out_uv) return SR_E_INVALID;
    sr::sky_uv(dir[0], dir[1], dir[2], HostAtan2(), HostAsin(), out_uv);
    return SR_OK;
}

// ---- ray queries (sr.h): caller-supplied rays through the current scene

namespace {
// What sr_trace_rays and sr_trace_ray_maps share: the checks of the context,
// the rays and the params in sr.h's order, the definition's frame, and the
// stream entered with the schedule's step table. outputs_ok: the caller's
// check of its own output pointers (at least one, each 4-byte aligned), which
// counts only when there are rays. *go false with SR_OK: nothing to launch.
int trace_prepare(sr_ctx* c, const float* dev_origins, const float* dev_dirs, int n_rays, const sr_params* p,
                  bool outputs_ok, hipStream_t s, sr_dev_frame& fr, const float4** tbl, bool* go) {
    *go = false;
    if (!c) return SR_E_INVALID;
    if (!c->scene_set) return SR_E_NOT_READY;
    if (n_rays < 0 || n_rays > SR_TRACE_MAX_RAYS) return SR_E_INVALID;
    // the definition's frame: 1 x 1, fov 90; the camera's position and forward
    // axis are each ray's own (geodesic.hip sr_trace_kernel), the rest is unread
    sr_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.fov = 90.0f;
    int rc = sr_pre::check_frame_args(&cam, p, 1, 1);
    if (rc != SR_OK) return rc;
    if (p->raytrace_type != SR_RAYTRACE_CURVED && p->raytrace_type != SR_RAYTRACE_FLAT) return SR_E_INVALID;  // no uv
    if (n_rays == 0) return SR_OK;
    if (!dev_origins || !dev_dirs || (((uintptr_t)dev_origins | (uintptr_t)dev_dirs) & 3) != 0) return SR_E_INVALID;
    if (!outputs_ok) return SR_E_INVALID;
    sr_params pp = *p;
    pp.crosshair = 0;
    pp.percent_black = -1.0f;
    sr_pre::derive_frame({&cam, 1, &pp, 1, 1, 1, nullptr, c->cull, SR_PROJECTION_RECTILINEAR}, c->h_scene, fr);
    // the one launch constant whose premise is the camera position ("chord
    // origins within r = 100"): the host cannot see the origins
    fr.win_ok = 0;
    // and the one about its direction: a frame's rays leave a camera that
    // looks at the scene, a trace launch's point anywhere, also along the
    // outward radius, where a coarse schedule's RK4 steps stop following the
    // orbit the outward lanes' exclusions assume (device_scene.h)
    if (!(fr.max_dphi <= SR_TRACE_DPHI_MAX)) fr.cull = 0;
    context_into_frame(c, true, fr);
    fr.fast_unroll = SR_FAST_UNROLL_DEFAULT;
    fr.tiles = 1;
    fr.nrows = 1;
    fr.block_rows = 1;
    // no pixel state, no launch order, no retained frame: the context's stay as they are
    rc = enter_stream(c, s);
    if (rc != SR_OK) return rc;
    rc = ensure_table(c, p->max_steps, p->max_revolutions, s, tbl);
    if (rc != SR_OK) return rc;
    *go = true;
    return SR_OK;
}
}  // namespace

int sr_trace_rays(sr_ctx* c, const float* dev_origins, const float* dev_dirs, int n_rays, const sr_params* p,
                  float* dev_rgba32, uint8_t* dev_rgba8, int32_t* dev_steps, int32_t* dev_ids, sr_stream stream) {
    const auto misaligned = [](const void* q) { return ((uintptr_t)q & 3) != 0; };
    const bool outputs_ok = (dev_rgba32 || dev_rgba8 || dev_steps || dev_ids) && !misaligned(dev_rgba32) &&
                            !misaligned(dev_rgba8) && !misaligned(dev_steps) && !misaligned(dev_ids);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    sr_dev_frame fr;
    const float4* tbl = nullptr;
    bool go = false;
    const int rc = trace_prepare(c, dev_origins, dev_dirs, n_rays, p, outputs_ok, s, fr, &tbl, &go);
    if (!go) return rc;
    return finish(c, sr_launch_trace(c->d_scene, tbl, c->d_segs, c->d_bg, c->d_arr, &fr, dev_origins, dev_dirs, n_rays,
                                     dev_rgba32, dev_rgba8, dev_steps, dev_ids, s),
                  s);
}

// ---- ray maps of ray queries (sr.h): sr_ray_maps' maps of sr_trace_rays' rays

int sr_trace_ray_maps(sr_ctx* c, const float* dev_origins, const float* dev_dirs, int n_rays, const sr_params* p,
                      const sr_ray_map_ptrs* m, sr_stream stream) {
    if (!c || !p || !m) return SR_E_INVALID;
    const void* const ptrs[9] = {m->end,        m->id,       m->sky_dir,  m->sky_uv,  m->hit_point,
                                 m->hit_normal, m->hit_view, m->hit_base, m->hit_step};
    bool any = false, aligned = true;
    for (const void* q : ptrs) {
        aligned = aligned && ((uintptr_t)q & 3) == 0;
        any = any || q != nullptr;
    }
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    sr_dev_frame fr;
    const float4* tbl = nullptr;
    bool go = false;
    const int rc = trace_prepare(c, dev_origins, dev_dirs, n_rays, p, any && aligned, s, fr, &tbl, &go);
    if (!go) return rc;
    return finish(c, sr_launch_trace_maps(c->d_scene, tbl, c->d_segs, c->d_arr, &fr, dev_origins, dev_dirs, n_rays, m, s),
                  s);
}

int sr_abi_struct_sizes(size_t* out, int n) {
    const size_t sz[6] = {sizeof(sr_camera), sizeof(sr_params), sizeof(sr_scene),
                          sizeof(sr_test_ray), sizeof(sr_material), sizeof(sr_light)};
    if (!out || n < 0) return SR_E_INVALID;
    for (int i = 0; i < n && i < 6; i++) out[i] = sz[i];
    return SR_OK;
}

int sr_set_split(sr_ctx* c, int max_tiles, int lanes_per_wave, int min_steps) {
    if (!c || max_tiles < 0 || max_tiles > (1 << 16) || min_steps < 0) return SR_E_INVALID;
    int lg;
    switch (lanes_per_wave) {
    case 16: lg = 4; break;
    case 4: lg = 2; break;
    case 1: lg = 0; break;
    default: return SR_E_INVALID;
    }
    c->split_tiles = max_tiles;
    c->split_log2 = lg;
    c->split_min_steps = min_steps;
    return SR_OK;
}

int sr_set_latency_mode(sr_ctx* c, int on) {
    if (!c) return SR_E_INVALID;
    c->fast_unroll = on ? 2 : SR_FAST_UNROLL_DEFAULT;
    return SR_OK;
}

// Host state alone: a launch copies it into its own frame struct, so frames
// in flight keep theirs and nothing is waited for. The launch orders are
// keyed by the projection (ensure_order).
int sr_set_projection(sr_ctx* c, int projection) {
    if (!c || projection < SR_PROJECTION_RECTILINEAR || projection > SR_PROJECTION_FISHEYE) return SR_E_INVALID;
    if (projection != c->projection) c->kept.valid = false;  // the retained call issued again would walk other rays
    c->projection = projection;
    return SR_OK;
}

int sr_get_projection(sr_ctx* c) { return c ? c->projection : SR_E_INVALID; }

namespace {
struct HostSin {
    float operator()(float x) const { return (float)std::sin((double)x); }
};
struct HostCos {
    float operator()(float x) const { return (float)std::cos((double)x); }
};
}  // namespace

int sr_projection_dir(int projection, float fov, int uv_width, int uv_height, int px, int py, float out_local[3]) {
    if (!out_local || uv_width <= 0 || uv_height <= 0 || px < 0 || py < 0 || px >= uv_width || py >= uv_height)
        return SR_E_INVALID;
    if (uv_width > INT32_MAX / 2 || uv_height > INT32_MAX / 2) return SR_E_INVALID;
    // sample_uv and init_pixel's uvv (geodesic.hip) for a plain frame of this size
    const float uvx = (float)(2 * px + 1) / (float)uv_width - 1.0f;
    const float uvy = (float)(2 * py + 1) / (float)uv_height - 1.0f;
    const float vy = uvy * (float)uv_height / (float)uv_width;
    const float a = sr::projection_half_angle(fov);
    const float fwd = 1.0f / (float)std::tan((double)a);  // precompute.cpp build_cam
    bool ray;
    switch (projection) {
    case SR_PROJECTION_RECTILINEAR:
        ray = sr::projection_local_dir<SR_PROJECTION_RECTILINEAR>(uvx, vy, a, fwd, HostSin(), HostCos(), out_local);
        break;
    case SR_PROJECTION_EQUIRECT:
        ray = sr::projection_local_dir<SR_PROJECTION_EQUIRECT>(uvx, vy, a, fwd, HostSin(), HostCos(), out_local);
        break;
    case SR_PROJECTION_FISHEYE:
        ray = sr::projection_local_dir<SR_PROJECTION_FISHEYE>(uvx, vy, a, fwd, HostSin(), HostCos(), out_local);
        break;
    default:
        return SR_E_INVALID;
    }
    return ray ? 1 : 0;
}

int sr_camera_rays(const sr_camera* cam, int projection, int width, int height, int row_begin, int row_end,
                   float* origins, float* dirs) {
    if (!cam || !origins || !dirs || width <= 0 || height <= 0 || bad_rows(row_begin, row_end, height))
        return SR_E_INVALID;
    if (width > INT32_MAX / 2 || height > INT32_MAX / 2) return SR_E_INVALID;
    if (projection < SR_PROJECTION_RECTILINEAR || projection > SR_PROJECTION_FISHEYE) return SR_E_INVALID;
    const float* a = cam->transform.axes;
    size_t k = 0;
    for (int py = row_begin; py < row_end; py++) {
        for (int px = 0; px < width; px++, k += 3) {
            float L[3];
            const int ray = sr_projection_dir(projection, cam->fov, width, height, px, py, L);
            if (ray < 0) return ray;
            for (int j = 0; j < 3; j++) {
                origins[k + j] = cam->transform.pos[j];
                // init_pixel's mv(axes, L) (geodesic.hip), before its normalize
                dirs[k + j] = ray ? (a[j] * L[0] + a[3 + j] * L[1]) + a[6 + j] * L[2] : NAN;
            }
        }
    }
    return SR_OK;
}

// Not in sr.h's public set: the launch codes order_tiles wrote at the end
// of the context's last frame (the next frame of that shape runs them; tile
// << 8, | 0x80 | sub for split workgroups, -1 unused). Waits for the frame.
int sr_debug_last_order(sr_ctx* c, int* out, int max_n, int* n) {
    if (!c || !n || max_n < 0 || (max_n && !out)) return SR_E_INVALID;
    const sr_cache::Caches& cc = c->caches;
    *n = (int)cc.last_slots;
    if (!cc.last_order) return SR_OK;
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    const size_t k = cc.last_slots < (size_t)max_n ? cc.last_slots : (size_t)max_n;
    if (k && (!hip_ok(hipMemcpyAsync(out, cc.last_order, k * sizeof(int), hipMemcpyDeviceToHost, c->upload)) ||
              !hip_ok(hipStreamSynchronize(c->upload))))
        return SR_E_HIP;
    return SR_OK;
}

// Not in sr.h's public set: a host copy of the integrate -> shade hand-off
// (geodesic.hip PS_*: SR_PS_FIELDS floats per pixel id in its planes) after
// the context's last frame, for post-mortems of single pixels without
// instrumenting the kernel. *n_px = pixel ids the buffer holds; copies
// min(max_floats, n_px * SR_PS_FIELDS) floats.
int sr_debug_pixel_state(sr_ctx* c, float* out, size_t max_floats, size_t* n_px) {
    if (!c || !n_px || (max_floats && !out)) return SR_E_INVALID;
    *n_px = c->ps_n();
    if (!max_floats || !c->d_ps()) return SR_OK;
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    size_t k = c->ps_n() * SR_PS_FIELDS;
    if (k > max_floats) k = max_floats;
    if (!hip_ok(hipMemcpyAsync(out, c->d_ps(), k * sizeof(float), hipMemcpyDeviceToHost, c->upload)) ||
        !hip_ok(hipStreamSynchronize(c->upload)))
        return SR_E_HIP;
    return SR_OK;
}

// Not in sr.h's public set: the retained launch's output shape for the
// bindings: out[0 .. 3] = width, rows and frames of its output, and its ss
// (1: plain). SR_E_NOT_READY without a retained frame.
int sr_debug_retained_shape(sr_ctx* c, int* out4) {
    if (!c || !out4) return SR_E_INVALID;
    if (!sr_can_reshade(c)) return SR_E_NOT_READY;
    const bool ss = c->kept.ss > 1;
    out4[0] = ss ? c->kept.width : c->kept.fr.width;
    out4[1] = ss ? c->kept.rows : c->kept.fr.nrows;
    out4[2] = c->kept.fr.batch;
    out4[3] = c->kept.ss;
    return SR_OK;
}

// Not in sr.h's public set: toggles segment culling (parity tests compare
// culled and exhaustive renders bit for bit).
int sr_debug_set_culling(sr_ctx* c, int enabled) {
    if (!c) return SR_E_INVALID;
    c->cull = enabled != 0;
    return SR_OK;
}

// Not in sr.h's public set: per-kernel HIP-event timing of the next
// `capacity` frames (0: off). bench.py reads the integrate kernel's duration
// for its roofline line from here.
int sr_debug_set_timing(sr_ctx* c, int capacity) {
    if (!c || capacity < 0 || capacity > (1 << 16)) return SR_E_INVALID;
    if (!hip_ok(hipSetDevice(c->device)) || !wait_ctx(c)) return SR_E_HIP;
    for (hipEvent_t e : c->tev) (void)hipEventDestroy(e);
    c->tev.assign(4 * (size_t)capacity, nullptr);
    c->timing_cap = 0;
    c->timing_n = 0;
    for (auto& e : c->tev)
        if (!hip_ok(hipEventCreate(&e))) return SR_E_HIP;
    c->timing_cap = capacity;
    return SR_OK;
}

// Waits for the recorded frames and writes ms[3 * f + j] (j = integrate,
// shade, resume) for up to max_frames of them; *n_frames = frames recorded.
// Restarts the recording.
int sr_debug_kernel_times(sr_ctx* c, float* ms, int max_frames, int* n_frames) {
    if (!c || !n_frames || max_frames < 0 || (max_frames && !ms)) return SR_E_INVALID;
    *n_frames = c->timing_n;
    const int n = c->timing_n < max_frames ? c->timing_n : max_frames;
    for (int f = 0; f < n; f++) {
        hipEvent_t* e = &c->tev[4 * (size_t)f];
        if (!hip_ok(hipEventSynchronize(e[3]))) return SR_E_HIP;
        for (int j = 0; j < 3; j++)
            if (!hip_ok(hipEventElapsedTime(&ms[3 * f + j], e[j], e[j + 1]))) return SR_E_HIP;
    }
    c->timing_n = 0;
    return SR_OK;
}

// ---- Not in sr.h's public set: the host precomputation without a device or
// a context, through the functions the entry points above pack with
// (tests/test_host_precompute.py holds their bytes to recorded digests).

// out[0 .. 2] = bytes of the scene image, of the segment buffer and of a frame struct
int sr_debug_precompute_sizes(size_t* out, int n) {
    const size_t sz[3] = {sizeof(sr_dev_scene), (size_t)SR_SEGS_BUF_FLOATS * sizeof(float), sizeof(sr_dev_frame)};
    if (!out || n < 0) return SR_E_INVALID;
    for (int i = 0; i < n && i < 3; i++) out[i] = sz[i];
    return SR_OK;
}

// What sr_set_scene(s) and sr_set_test_ray(t) would upload on a fresh context
// (null s: no scene yet; null t: sr_create's default test ray). Their status;
// the buffers are written on SR_OK only.
int sr_debug_pack_scene(const sr_scene* s, const sr_test_ray* t, void* scene_out, float* segs_out) {
    if (!scene_out || !segs_out) return SR_E_INVALID;
    sr_dev_scene d;
    std::vector<float> segs;
    const int rc = fresh_image(s, t, d, segs);
    if (rc != SR_OK) return rc;
    std::memcpy(scene_out, &d, sizeof d);
    std::memcpy(segs_out, segs.data(), segs.size() * sizeof(float));
    return SR_OK;
}

// The frame struct a whole-frame sr_render would build on that context
// (culling and the projection as given, every other setting at its default,
// no textures; the pointer fields are null). The launch's status.
int sr_debug_frame(const sr_scene* s, const sr_test_ray* t, const sr_camera* cam, const sr_params* p, int width,
                   int height, int cull, int projection, void* frame_out) {
    if (!frame_out) return SR_E_INVALID;
    sr_ctx c;
    std::vector<float> segs;
    int rc = fresh_image(s, t, c.h_scene, segs);
    if (rc != SR_OK) return rc;
    c.scene_set = s != nullptr;
    c.cull = cull != 0;
    c.projection = projection;
    sr_dev_frame fr;
    rc = build_frame(&c, Launch(cam, 1, p, width, height, nullptr).band(0, height).into(nullptr, (size_t)width * 4),
                     fr);
    if (rc == SR_OK) std::memcpy(frame_out, &fr, sizeof fr);
    return rc;
}

// The shutter resolve's division as the kernel computes it (kernels/shutter_div.h):
// n div k for n < 2^16, k in 1 .. 256; -1 outside
int sr_debug_shutter_div(int n, int k) {
    if (n < 0 || n > 0xffff || k < 1 || k > 256) return -1;
    return (int)sr_shutter_div((uint32_t)n, sr_shutter_magic((uint32_t)k));
}

// The step table of a schedule: 4 * (max_steps + 4) floats
int sr_debug_step_table(int max_steps, int max_revolutions, float* out, size_t n_floats) {
    if (!out || max_steps < 0 || max_steps > SR_MAX_STEPS || n_floats != 4 * ((size_t)max_steps + 4)) return SR_E_INVALID;
    const std::vector<sr_pre::StepEntry> t = sr_pre::step_table(max_steps, max_revolutions);
    std::memcpy(out, t.data(), n_floats * sizeof(float));
    return SR_OK;
}

// The opacity bitmap of a texture array: ceil(w / 8) * h * layers bytes
int sr_debug_opacity_bits(const uint8_t* px, int w, int h, int layers, int ch, uint8_t* out, size_t bytes) {
    if (!px || !out || w <= 0 || h <= 0 || layers <= 0 || (ch != 3 && ch != 4)) return SR_E_INVALID;
    const std::vector<uint8_t> bits = sr_pre::opacity_bits(px, w, h, layers, ch);
    if (bits.size() != bytes) return SR_E_INVALID;
    std::memcpy(out, bits.data(), bytes);
    return SR_OK;
}

}  // extern "C"
