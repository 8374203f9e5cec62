/*
 * sr.h — C-ABI of the MI355X-native Schwarzschild geodesic renderer.
 *
 * This is the drop-in boundary that replaces the reference's GL shader-program
 * interface (Yachim/schwarzschild-raytracer):
 *
 *   reference                                              replaced by
 *   -----------------------------------------------------  -------------------------
 *   glDrawElements(full-screen quad)  src/main.cpp:318-319  sr_render / sr_render_blocks
 *   Camera::loadShader                camera.cpp:41-50      sr_camera argument
 *   ObjectLoader::load                objectLoader.cpp:27   sr_set_scene (snapshot)
 *   loadTexture(bg) + unit 0          image_utils.cpp:7-40  sr_set_background
 *   loadTextureArray + unit 1         image_utils.cpp:42    sr_set_texture_array
 *   glUniform percent_black/max_steps src/main.cpp:295-297  sr_params
 *   glUniform raytrace_type/...       src/main.cpp:394-427  sr_params
 *   test-ray uniforms (press R)       src/main.cpp:375-391  sr_set_test_ray
 *   calculateTestRayPoints            src/main.cpp:94-124   sr_test_ray_points
 *
 * The structs below are POD mirrors of the GLSL uniform block of
 * assets/shaders/black_hole.frag:15-192: same field names, same capacities.
 * Matrices are column-major 3x3 exactly as uploaded by
 * glUniformMatrix3fv(..., GL_FALSE, &m_axes[0].x) (transform.cpp:67-68):
 * axes[0..2] = column 0 (right), axes[3..5] = column 1 (up),
 * axes[6..8] = column 2 (forward).
 *
 * Conventions: extern "C", no exceptions cross the ABI, every call returns an
 * sr_status (0 = ok, < 0 = error). A context is bound to one HIP device and is
 * not thread-safe (one host thread per context), like the reference's single
 * GL context (SURVEY §8b "Threading").
 */
#ifndef SR_SR_H
#define SR_SR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Capacities — black_hole.frag:63,67,88,96,113,121,130,140,149,159,178,182 */
#define SR_MAX_LIGHTS       4
#define SR_MAX_TEXTURES     10
#define SR_MAX_MATERIALS    10
#define SR_MAX_SPHERES      3
#define SR_MAX_PLANES       3
#define SR_MAX_DISKS        3
#define SR_MAX_HOLLOW_DISKS 3
#define SR_MAX_CYLINDERS    3
#define SR_MAX_RECTANGLES   3
#define SR_MAX_BOXES        3
#define SR_MAX_OBJECTS      21
#define SR_MAX_POINTS       1000
/* max_steps limit: the integrate -> shade hand-off packs a ray's step count into 24 bits */
#define SR_MAX_STEPS        ((1 << 24) - 1)

/* Object type codes — black_hole.frag:162-171 == ObjectType (object.h:7-19) */
#define SR_OBJECT_SPHERE      0
#define SR_OBJECT_PLANE       1
#define SR_OBJECT_DISK        2
#define SR_OBJECT_HOLLOW_DISK 3
#define SR_OBJECT_CYLINDER    4 /* ObjectType::LATERAL_CYLINDER */
#define SR_OBJECT_RECTANGLE   5
#define SR_OBJECT_BOX         6

/* Raytrace modes — black_hole.frag:32-35 == RaytraceType (camera.h:14-19) */
#define SR_RAYTRACE_CURVED      0
#define SR_RAYTRACE_FLAT        1
#define SR_RAYTRACE_HALF_WIDTH  2
#define SR_RAYTRACE_HALF_HEIGHT 3

/* Bilinear filter arithmetic. The GL spec leaves the weight
 * arithmetic to the implementation; it decides whether an opaque textured hit
 * reaches alpha == 1.0 exactly (black_hole.frag:932).
 *   SR_FILTER_LERP     : lerp form, exactly 1.0 on all-opaque texels (hardware TMU-like).
 *   SR_FILTER_WEIGHTED : four-weight sum (SwiftShader-like; may give 0.99999994). */
#define SR_FILTER_LERP     0
#define SR_FILTER_WEIGHTED 1

typedef enum {
    SR_OK = 0,
    SR_E_INVALID = -1,   /* bad argument (null pointer, bad size, bad mode) */
    SR_E_CAPACITY = -2,  /* more objects/lights/... than the GLSL arrays hold */
    SR_E_HIP = -3,       /* a HIP runtime call failed */
    SR_E_NOMEM = -4,     /* host or device allocation failed */
    SR_E_NOT_READY = -5, /* sr_render before sr_set_scene */
    SR_E_NO_DEVICE = -6, /* no HIP device / bad device ordinal */
    SR_E_IO = -7         /* a file could not be written (sr_write_png) */
} sr_status;

/* struct Transform — black_hole.frag:41-44 */
typedef struct {
    float pos[3];
    float axes[9]; /* column-major: right, up, forward */
} sr_transform;

/* struct Camera — black_hole.frag:46-49 (fov: horizontal, degrees) */
typedef struct {
    sr_transform transform;
    float fov;
} sr_camera;

/* struct Light — black_hole.frag:54-61 */
typedef struct {
    sr_transform transform;
    float color[3];
    float intensity;
    float attenuation_constant;
    float attenuation_linear;
    float attenuation_quadratic;
} sr_light;

/* struct Material — black_hole.frag:72-86 (bools as int32) */
typedef struct {
    float color[4];
    float ambient;
    float diffuse;
    float specular;
    float shininess;
    int32_t texture_index;    /* < 0 disables */
    int32_t normal_map_index; /* < 0 disables */
    int32_t invert_uv_x;
    int32_t invert_uv_y;
    int32_t swap_uvs;
    int32_t double_sided_normals;
    int32_t flip_normals;
} sr_material;

/* struct Sphere — black_hole.frag:91-94 */
typedef struct {
    sr_transform transform;
    float radius;
} sr_sphere;

/* struct Plane — black_hole.frag:106-111 */
typedef struct {
    sr_transform transform;
    float texture_offset[2];
    int32_t repeat_texture;
    float texture_size[2];
} sr_plane;

/* struct Disk — black_hole.frag:116-119 */
typedef struct {
    sr_plane plane;
    float radius;
} sr_disk;

/* struct HollowDisk — black_hole.frag:124-128 */
typedef struct {
    sr_plane plane;
    float inner_radius;
    float outer_radius;
} sr_hollow_disk;

/* struct Cylinder (lateral surface only) — black_hole.frag:134-138 */
typedef struct {
    sr_transform transform;
    float height;
    float radius;
} sr_cylinder;

/* struct Rectangle — black_hole.frag:143-147 */
typedef struct {
    sr_plane plane;
    float width;
    float height;
} sr_rectangle;

/* struct Box — black_hole.frag:152-157 */
typedef struct {
    sr_transform transform;
    float width;
    float depth;
    float height;
} sr_box;

/* struct Object — black_hole.frag:172-176 */
typedef struct {
    int32_t type;
    int32_t index;          /* into the per-type array */
    int32_t material_index; /* into materials[]; ObjectLoader starts at 1 */
} sr_object;

/* The scene half of the uniform block (what ObjectLoader::load and
 * loadTextureArray upload once): black_hole.frag:64-65, 68-69, 89, 97-160,
 * 179-180. */
typedef struct {
    int32_t num_objects;
    sr_object objects[SR_MAX_OBJECTS];
    sr_sphere spheres[SR_MAX_SPHERES];
    sr_plane planes[SR_MAX_PLANES];
    sr_disk disks[SR_MAX_DISKS];
    sr_hollow_disk hollow_disks[SR_MAX_HOLLOW_DISKS];
    sr_cylinder cylinders[SR_MAX_CYLINDERS];
    sr_rectangle rectangles[SR_MAX_RECTANGLES];
    sr_box boxes[SR_MAX_BOXES];
    sr_material materials[SR_MAX_MATERIALS];
    int32_t num_lights;
    sr_light lights[SR_MAX_LIGHTS];
    float texture_sizes[SR_MAX_TEXTURES][2];
    float max_texture_size[2];
} sr_scene;

/* Per-frame parameters: black_hole.frag:15-39 uniforms. Defaults (sr_params_default)
 * are the shader's initializers, with max_revolutions = 2 (the app's glUniform1f
 * upload into an int uniform is rejected, src/main.cpp:297). */
typedef struct {
    int32_t max_steps;          /* frag:19 */
    int32_t max_revolutions;    /* frag:20 */
    float u_f;                  /* frag:22 */
    int32_t crosshair;          /* frag:24 */
    int32_t raytrace_type;      /* frag:36 */
    float curved_percentage;    /* frag:37 */
    float percent_black;        /* frag:39; < 0 disables the noise mask */
    float time;                 /* frag:16 (declared, unused by the shader) */
    int32_t filter_mode;        /* SR_FILTER_* (texture() arithmetic) */
} sr_params;

/* Test-ray overlay uniforms: black_hole.frag:182-192 (set on key R, src/main.cpp:375-391). */
typedef struct {
    int32_t visible;                  /* test_ray_visible */
    float radius;                     /* test_ray_radius (0.025) */
    float extended_length;            /* test_ray_extended_length (1000) */
    float curved_color[4];            /* (1,0,0,1) */
    float flat_color[4];              /* (0,1,0,1) */
    float flat_origin[3];
    float flat_dir[3];
    int32_t num_curved_points;
    float curved_points[SR_MAX_POINTS][3];
} sr_test_ray;

typedef struct sr_ctx sr_ctx;
typedef struct ihipStream_t* sr_stream; /* == hipStream_t; NULL = default stream */

/* Library / defaults -------------------------------------------------------- */
const char* sr_version(void);
const char* sr_status_string(int status);
void sr_params_default(sr_params* out);
void sr_test_ray_default(sr_test_ray* out);
void sr_scene_clear(sr_scene* out);
/* The app's hard-coded scene and camera (src/main.cpp:222-268), textures
 * described by texture_sizes (uv_checker 600x600, cubemap 1601x1201). */
void sr_default_scene(sr_scene* out);
void sr_default_camera(sr_camera* out);
/* The app's H-key flyby (src/main.cpp:404-410 -> Camera::hyperbolicTrajectory,
 * camera.cpp:20-33, then lookAt(origin), camera.cpp:35-39): moves *cam along
 * the hyperbola of the given initial / closest distance at eased time t in
 * [0, 1] (the app: 30, 10, elapsed / HYPERBOLIC_TRAJECTORY_DURATION). The fov
 * is kept. Host-only, per frame. */
int sr_camera_hyperbolic_trajectory(sr_camera* cam, float initial_distance, float closest_distance,
                                    float time);

/* Context ------------------------------------------------------------------- */
int sr_create(sr_ctx** out, int hip_device);
void sr_destroy(sr_ctx* ctx);

/* Skybox: already flipped as stbi_set_flip_vertically_on_load(true) leaves it
 * (row 0 = v 0). channels 3 (GL_RGB: alpha reads 1) or 4. Synchronous copy. */
int sr_set_background(sr_ctx* ctx, const uint8_t* pixels, int width, int height, int channels);
/* Texture array image exactly as glTexImage3D receives it (already padded to the
 * max size; layer-major, rows bottom-up). channels 3 or 4. */
int sr_set_texture_array(sr_ctx* ctx, const uint8_t* pixels, int width, int height,
                         int layers, int channels);
/* Snapshot copy of the scene (ObjectLoader::load semantics). Validates types,
 * per-type indices and material indices: SR_E_CAPACITY instead of the
 * reference's silent glUniform drop. */
int sr_set_scene(sr_ctx* ctx, const sr_scene* scene);
int sr_set_test_ray(sr_ctx* ctx, const sr_test_ray* test_ray);

/* Render rows [row_begin, row_end) of a width x height frame (GL order: row 0
 * is the bottom row) into dev_rgba8 (device memory, row r at
 * dev_rgba8 + (r - row_begin) * pitch_bytes). Asynchronous on `stream`.
 * A context reuses its per-frame scratch (pixel state, launch order), so its
 * renders are ordered: a launch on another stream than the context's last
 * one first waits (hipStreamWaitEvent on an event recorded at the end of that
 * launch) for the work of that stream. Between launches the context frees
 * replaced buffers in stream order on its last launch's stream, and the calls
 * that wait for the context's frames (sr_set_*, sr_wave_costs, sr_destroy)
 * synchronise it: keep that stream alive until the context's next launch (on
 * any stream) or sr_destroy. */
int sr_render(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width,
              int height, int row_begin, int row_end, uint8_t* dev_rgba8,
              size_t pitch_bytes, sr_stream stream);

/* Block-cyclic row bands for multi-GPU tiling: frame rows are cut in blocks of
 * `block_rows`; this call renders blocks b = block_first + k*block_step
 * (k = 0, 1, ...) and packs them densely: block k's row j lands at
 * dev_rgba8 + (k*block_rows + j) * pitch_bytes. */
int sr_render_blocks(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width,
                     int height, int block_rows, int block_first, int block_step,
                     uint8_t* dev_rgba8, size_t pitch_bytes, sr_stream stream);

/* Frames in one launch (not in the reference; the pixels are unchanged): the
 * rows sr_render_blocks would render, for n_frames (1 .. 32) frames that
 * differ only in the camera (cams[f]), frame f packed at dev_rgba8 + f *
 * frame_stride_bytes. One launch carries n_frames times the work, so a GPU
 * holding a small share of each frame (multi-GPU row tiling) runs it as
 * efficiently as a whole frame; the launch order and split tiles follow the
 * costliest tiles over the batch. SR_E_CAPACITY above 32 frames. */
int sr_render_blocks_batch(sr_ctx* ctx, const sr_camera* cams, int n_frames, const sr_params* params,
                           int width, int height, int block_rows, int block_first, int block_step,
                           uint8_t* dev_rgba8, size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);

/* A rank's cost-balanced rows (not in the reference; the pixels are
 * unchanged): like sr_render_blocks_batch, but output row k of each frame's
 * tile renders frame row blocks[k / block_rows] * block_rows + k % block_rows
 * for an explicit list of n_blocks block indices (-1: padding, rows left
 * unwritten). The list is copied to the device once per distinct list and
 * kept with the context. schwarzschild-raytracer_amd/dist.py balanced_blocks
 * builds equal-length lists of about equal cost for the ranks of a node. */
int sr_render_block_list(sr_ctx* ctx, const sr_camera* cams, int n_frames, const sr_params* params, int width,
                         int height, int block_rows, const int* blocks, int n_blocks, uint8_t* dev_rgba8,
                         size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);

/* Per-wave cost map of one whole frame (not in the reference), for
 * cost-balanced multi-GPU shares: renders the frame (no image output, split
 * tiles off for this launch) and writes, for each 8x8 wave tile (row block
 * b = y / 8, column c = x / 8), dev_out[(b * ceil(width / 8) + c) * 2] = the
 * wave's longest ray's executed steps (a ray whose hit log filled counts with
 * the steps the resume kernel ran for it too) and [... + 1] = its budget events
 * (DESIGN.md §5): int32 [ceil(height / 8)][ceil(width / 8)][2]. Deterministic,
 * so every rank of a node derives the same block lists from it. The map comes
 * from a culling kernel whatever the params: with max_revolutions <= 0 or a
 * negative or NaN u_f, whose frames are rendered without culling (DESIGN.md
 * §5), it is an estimate of their cost only. No pixel is written by this call. */
int sr_wave_costs(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width, int height,
                  int32_t* dev_out, sr_stream stream);

/* ---- Multi-GPU frame partition (not in the reference, whose frame is one
 * draw on one GPU, src/main.cpp:318-319). A frame's rows are cut
 * into blocks of block_rows (8: one 8x8 wave tile tall); every rank of a node
 * renders an equal-length list of blocks of about equal cost with
 * sr_render_block_list, the tiles are gathered to the root (the caller's
 * RCCL collective: ncclGather of equal-size tiles, examples/sr_multi_gpu.cpp)
 * and sr_assemble_blocks puts the frame back together. */

/* Per-block cost from an sr_wave_costs map copied to the host
 * ([n_blocks][waves_per_block][2] = {steps, events} per 8x8 wave): out_cost[b]
 * = sum over the block's waves of steps + event_steps x events (a wave runs
 * until its longest ray ends; a budget event costs about 8 wave-steps,
 * DESIGN.md §8). Same values as dist.block_costs. */
int sr_block_costs(const int32_t* wave_cost, int n_blocks, int waves_per_block, double event_steps,
                   double* out_cost);

/* Equal-length block lists of about equal cost for `world` ranks:
 * out_lists[r * per + s] (-1: padding), *out_per = ceil(n_blocks / world);
 * SR_E_CAPACITY when world * per > max_entries. Blocks by descending cost to
 * the least-loaded rank with room, then pairwise swaps out of the most
 * loaded rank while one lowers the pair's maximum; the block-cyclic lists
 * when they are at least as even. Deterministic, binary64, the same lists as
 * dist.balanced_blocks: every rank derives identical lists from identical
 * costs (or the root computes and broadcasts them). */
int sr_balanced_blocks(const double* cost, int n_blocks, int world, int* out_lists, int max_entries, int* out_per);

/* Reassembles n_frames frames from gathered tiles: rank r's tile of frame f
 * starts at stacked + r * rank_stride + f * in_frame_stride, its slot s holds
 * the block_rows rows of frame block lists[r * per + s] (dense rows of
 * row_bytes); frame f's row y lands at out + f * out_frame_stride + y *
 * row_bytes (rows >= height dropped, -1 slots skipped). on_device != 0: every
 * pointer, `lists` included, is device memory and the copy is a kernel on
 * `stream` (asynchronous); 0: host memory, synchronous. */
int sr_assemble_blocks(const uint8_t* stacked, size_t rank_stride, size_t in_frame_stride, const int* lists,
                       int world, int per, int height, int block_rows, size_t row_bytes, uint8_t* out,
                       size_t out_frame_stride, int n_frames, int on_device, sr_stream stream);

/* ---- Supersampling (not in the reference, whose shader takes one sample at
 * each pixel centre): an ordered grid of ss x ss samples per pixel, ss in
 * 1 .. SR_MAX_SUPERSAMPLE, with a box resolve. The sample frame S is exactly
 * the frame this library renders for (ss * width) x (ss * height) with the
 * same scene, camera (the fov is horizontal, so the framing is the same),
 * params, textures and test ray. Output pixel (x, y), channel c:
 *
 *   out[y][x][c] = (sum_{j < ss} sum_{i < ss} S[ss*y + j][ss*x + i][c] + (ss*ss) / 2) div (ss*ss)
 *
 * in integers on S's RGBA8 bytes ((ss*ss) / 2 = 0, 2, 4, 8), all four
 * channels alike. The sum does not depend on its order, so every
 * implementation of the rule gives the same bits. By that definition:
 *  - the crosshair (params.crosshair) is drawn in the sample frame and comes
 *    out 1 / ss the size (a caller who wants a fixed size draws their own);
 *  - the noise mask (percent_black) and the split modes (raytrace_type) are
 *    evaluated per sample;
 *  - ss == 1 is the plain frame, byte for byte (no scratch, no resolve).
 * sr_set_split, sr_set_latency_mode and the learned launch order apply to the
 * sample frame as to any frame of its size.
 *
 * Scratch: a context keeps one sample buffer, grown on demand in stream order
 * on the launch's stream and released by sr_destroy, of
 *   4 * ss*ss * width * rows * n_frames bytes
 * for the largest launch so far (rows: the output rows of the call's tile;
 * 33 MB for one 1920x1080 frame at ss 2, 4.2 GB for 32 of them at ss 4).
 * SR_E_NOMEM, with nothing launched, when it cannot be allocated. The resolve
 * runs on the same stream after the sample launch. */
#define SR_MAX_SUPERSAMPLE 4

/* sr_render with supersampling: rows [row_begin, row_end) of the width x
 * height output frame, each pixel from ss x ss samples. SR_E_INVALID for ss
 * outside 1 .. SR_MAX_SUPERSAMPLE, or more than 2^24 sample rows. */
int sr_render_ss(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width, int height,
                 int row_begin, int row_end, int ss, uint8_t* dev_rgba8, size_t pitch_bytes,
                 sr_stream stream);

/* sr_render_block_list with supersampling: the same layout (n_frames cameras,
 * an explicit block list, -1 padding and the rows past the frame's last row
 * left unwritten), width, height, block_rows, pitch and frame stride all
 * those of the OUTPUT frame, so a rank's tile has the shape
 * sr_assemble_blocks expects. SR_E_INVALID when ss * n_blocks * block_rows
 * exceeds 2^24 rows. dist.supersample_block_costs prices the output blocks
 * from an sr_wave_costs map of the sample frame. */
int sr_render_block_list_ss(sr_ctx* ctx, const sr_camera* cams, int n_frames, const sr_params* params,
                            int width, int height, int block_rows, const int* blocks, int n_blocks,
                            int ss, uint8_t* dev_rgba8, size_t pitch_bytes,
                            size_t frame_stride_bytes, sr_stream stream);

/* The resolve alone: n_frames sample images of (ss * width) x (ss * rows)
 * (row r at samples + f * sample_frame_stride + r * sample_pitch) to width x
 * rows images by the rule above. on_device != 0: device pointers, a kernel
 * on `stream`, asynchronous (vector loads when the sample pointer, pitch and
 * stride are multiples of 8 / 4 / 16 bytes for ss 2 / 3 / 4 and the output's
 * of 4, a byte path otherwise); 0: host memory, synchronous (the same rule
 * in plain C++). */
int sr_resolve_box(const uint8_t* samples, size_t sample_pitch, size_t sample_frame_stride,
                   int width, int rows, int ss, uint8_t* out, size_t pitch, size_t out_frame_stride,
                   int n_frames, int on_device, sr_stream stream);

/* ---- Sample phases and progressive supersampling (not in the reference). S
 * is the sample frame exactly as sr_render_ss defines it: the frame this
 * library renders for (ss * width) x (ss * height) with the same scene,
 * camera, params, textures and test ray, ss in 1 .. SR_MAX_SUPERSAMPLE.
 *
 * Phase image: phase (i, j), i and j in 0 .. ss - 1, is the width x height
 * image of one sub-sample position of every output pixel,
 *
 *   phase(i, j)[y][x] = S[ss*y + j][ss*x + i]     (all four bytes)
 *
 *  - the crosshair, the noise mask (percent_black) and the split modes
 *    (raytrace_type) are those of S, evaluated at the sample's own position;
 *  - ss == 1, phase (0, 0) is the plain frame, byte for byte.
 * A phase launch has the grid, the pixel state (208 bytes per OUTPUT pixel)
 * and the launch order of a plain width x rows frame: the order is the one
 * cached for that shape, shared with plain frames of it, learned and used as
 * sr_render does; sr_set_split, sr_set_latency_mode and culling apply as to
 * any frame of that size.
 *
 * Accumulator: caller-owned memory, uint16_t[rows][width][4] (row r at
 * accum + r * accum_pitch_bytes); base address and pitch must be multiples
 * of 8. RGBA8 images are added channel by channel in plain 16-bit adds
 * (modulo 2^16): SR_MAX_ACCUM_PASSES (256) images cannot wrap, 256 * 255 fits.
 *
 * Resolve: out[y][x][c] = min(255, (acc[y][x][c] + n / 2) div n) in integers,
 * n in 1 .. SR_MAX_ACCUM_PASSES. With n = ss * ss over all phases of a grid
 * this is the box rule above: the result equals sr_render_ss's frame byte for
 * byte, in whatever order and grouping the phases were added. Any prefix of
 * the phases resolved with its own count is a displayable frame, each pass at
 * about the cost of one plain frame, and one phase at a time needs no more
 * memory than a plain frame plus the accumulator, at any ss. */
#define SR_MAX_ACCUM_PASSES 256

/* sr_render with the phase mapping: rows [row_begin, row_end) of phase
 * (phase_x, phase_y) of the ss x ss grid. No scratch beyond a plain frame's.
 * SR_E_INVALID for ss outside 1 .. SR_MAX_SUPERSAMPLE or a phase coordinate
 * outside 0 .. ss - 1; otherwise as sr_render. */
int sr_render_phase(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width, int height,
                    int row_begin, int row_end, int ss, int phase_x, int phase_y, uint8_t* dev_rgba8,
                    size_t pitch_bytes, sr_stream stream);

/* Renders n_phases (1 .. 32) phases of one camera in ONE launch (the frames
 * of a batch, as sr_render_blocks_batch carries cameras) and adds them to the
 * accumulator's rows [0, row_end - row_begin) (reset != 0: stores their sum
 * instead, the accumulator is not read), all asynchronous on `stream` with no
 * host synchronisation. phases: n_phases pairs of bytes {x, y} (host memory,
 * read during the call). Scratch: the context's sample buffer (see above),
 * 4 * width * rows * n_phases bytes, and the pixel state of n_phases plain
 * frames. SR_E_INVALID for ss outside 1 .. SR_MAX_SUPERSAMPLE, a phase
 * coordinate outside 0 .. ss - 1, null pointers, n_phases < 1,
 * accum_pitch_bytes < 8 * width or a misaligned accumulator; SR_E_CAPACITY
 * above 32 phases; SR_E_NOT_READY and SR_E_NOMEM (nothing launched) as for
 * sr_render_ss. */
int sr_render_accumulate(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width, int height,
                         int row_begin, int row_end, int ss, const uint8_t* phases, int n_phases, int reset,
                         uint16_t* dev_accum, size_t accum_pitch_bytes, sr_stream stream);

/* The add alone: n_images (1 .. SR_MAX_ACCUM_PASSES) RGBA8 images of width x
 * rows (row r of image k at images + k * image_stride + r * pitch; the
 * pointer, pitch and stride multiples of 4) added to the accumulator, or
 * stored when reset != 0. on_device != 0: device pointers, a kernel on
 * `stream`, asynchronous; 0: host memory, synchronous (the same rule in plain
 * C++). SR_E_INVALID for null pointers, sizes <= 0, a short pitch or stride,
 * a misaligned pointer or n_images out of range. */
int sr_accum_add(const uint8_t* images, size_t pitch, size_t image_stride, int n_images, int width, int rows,
                 int reset, uint16_t* accum, size_t accum_pitch, int on_device, sr_stream stream);

/* The resolve alone, by the rule above, into RGBA8 rows (out and pitch
 * multiples of 4). on_device as for sr_accum_add. SR_E_INVALID for null
 * pointers, sizes <= 0, a short pitch, a misaligned pointer or n outside
 * 1 .. SR_MAX_ACCUM_PASSES. */
int sr_accum_resolve(const uint16_t* accum, size_t accum_pitch, int width, int rows, int n, uint8_t* out,
                     size_t pitch, int on_device, sr_stream stream);

/* Progressive order (host only): pass k (0 .. ss*ss - 1) of an ss x ss grid
 * renders phase (*phase_x, *phase_y); every prefix spreads over the pixel:
 *   ss 1: (0,0)
 *   ss 2: (0,0) (1,1) (1,0) (0,1)
 *   ss 3: (1,1) (0,0) (2,2) (2,0) (0,2) (1,0) (1,2) (0,1) (2,1)
 *   ss 4: (0,0) (2,2) (2,0) (0,2) (1,1) (3,3) (3,1) (1,3)
 *         (1,0) (3,2) (3,0) (1,2) (0,1) (2,3) (2,1) (0,3)
 * (ss 2 and 4: the 2x2 and 4x4 ordered-dither matrices read by rank).
 * SR_E_INVALID for ss or k out of range or a null pointer. */
int sr_phase_order(int ss, int k, int* phase_x, int* phase_y);

/* ---- Adaptive supersampling (not in the reference): supersample only the
 * 16x16 output tiles of the frame that hold an edge. Inputs: one camera and
 * one whole width x height frame, ss in 2 .. SR_MAX_SUPERSAMPLE, threshold
 * (int), grow in 0 .. 2. Byte-exact, no tolerance anywhere:
 *
 *  - P is the plain width x height frame, exactly what sr_render writes; S the
 *    (ss * width) x (ss * height) sample frame exactly as sr_render_ss defines
 *    it; R is S's box resolve by the rule above.
 *  - Output tile (tx, ty) covers pixels x in [16 tx, 16 tx + 15] and y in
 *    [16 ty, 16 ty + 15], clipped to the frame: ceil(width / 16) x
 *    ceil(height / 16) tiles. An output tile is exactly the ss x ss block
 *    (ss tx + i, ss ty + j) of the sample frame's own 16x16 workgroup tiles,
 *    for every ss (the ones past the sample grid's edge on a partial tile do
 *    not exist).
 *  - Edge rule, on P's RGBA8 bytes, all four channels alike: two pixels that
 *    are horizontal or vertical neighbours inside the frame form an edge pair
 *    when max over c of |a_c - b_c| > threshold. A tile is seeded when a pixel
 *    of it belongs to an edge pair; a pair that straddles a tile boundary
 *    seeds both tiles. threshold < 0 seeds every tile, threshold >= 255 none.
 *  - The flagged set is the seeded set dilated `grow` times by the 3x3
 *    (Chebyshev) neighbourhood on the tile grid.
 *  - out[y][x] = R[y][x] when pixel (x, y)'s tile is flagged, else P[y][x].
 *
 * By that definition:
 *  - the crosshair, the noise mask (percent_black) and the split modes
 *    (raytrace_type) follow P in an unflagged tile and S in a flagged one; a
 *    noise mask therefore flags nearly everything;
 *  - a feature thinner than a pixel that P misses entirely is not found:
 *    `grow` is the knob for that;
 *  - with threshold < 0 the output equals sr_render_ss's, byte for byte;
 *  - with threshold >= 255 it equals sr_render's, and no sample work is
 *    launched.
 *
 * sr_render_adaptive renders P into dev_rgba8 with the ordinary launch (which
 * runs and learns the launch order as sr_render does), selects the tiles
 * with a kernel, launches the sample frame for the flagged tiles only and
 * resolves them over P, all asynchronous on `stream` with no host
 * synchronisation anywhere in the call. sr_set_latency_mode and culling apply
 * to the sample launch; sr_set_split does not, and no launch order is learned
 * from it or for it (its tiles run in the order the plain frame just learned,
 * costliest first). Whole frames only, one camera: row bands, block
 * lists, batches and the multi-GPU path are out of scope. dev_tile_mask (may
 * be NULL; device memory, [ceil(height / 16)][ceil(width / 16)] bytes 0 / 1)
 * receives the flagged set. Scratch: the sample buffer and the pixel state of
 * the whole sample frame, as for sr_render_ss of the frame (4 and 208 bytes
 * per sample), and 1 + 4 ss^2 bytes per tile; all kept by the context, grown
 * in stream order, released by sr_destroy. SR_E_INVALID for ss outside
 * 2 .. SR_MAX_SUPERSAMPLE, grow outside 0 .. 2, a null output, pitch_bytes <
 * 4 * width, or more than 2^24 sample rows; SR_E_NOT_READY and SR_E_NOMEM
 * (nothing launched) as for sr_render_ss. */
int sr_render_adaptive(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width, int height,
                       int ss, int threshold, int grow, uint8_t* dev_rgba8, size_t pitch_bytes,
                       uint8_t* dev_tile_mask, sr_stream stream);

/* The selection alone: the flagged set of a width x height RGBA8 image (row y
 * at rgba8 + y * pitch) by the edge rule and `grow` above into
 * tile_mask[ceil(height / 16)][ceil(width / 16)], bytes 0 / 1. on_device !=
 * 0: device pointers, kernels on `stream`, asynchronous; 0: host memory,
 * synchronous (the same rule in plain C++). SR_E_INVALID for null pointers,
 * sizes <= 0, pitch < 4 * width or grow outside 0 .. 2. */
int sr_edge_tiles(const uint8_t* rgba8, size_t pitch, int width, int height, int threshold, int grow,
                  uint8_t* tile_mask, int on_device, sr_stream stream);

/* Debug/parity variant: unclamped FragColor as float RGBA (dev_rgba32, may be
 * NULL), the RGBA8 pixel (dev_rgba8, may be NULL) and the number of executed
 * geodesic steps per pixel (dev_steps, may be NULL). Dense rows. */
int sr_render_debug(sr_ctx* ctx, const sr_camera* cam, const sr_params* params, int width,
                    int height, int row_begin, int row_end, float* dev_rgba32,
                    uint8_t* dev_rgba8, int32_t* dev_steps, sr_stream stream);

/* ---- Retained frames (not in the reference, which walks every geodesic again
 * for every draw). A launch leaves a record per pixel: how the ray ended, its
 * final direction, its logged hits (point, object, step count) and, where the
 * log filled, the state to resume from. The record depends on the geometry,
 * the camera, the params, the test ray and the hits' opacity only; lights,
 * Phong terms, a colour's rgb, normal maps and the skybox never reach the
 * integrate kernel. The context remembers what its pixel state holds, the
 * retained frame, and for how long it stays true.
 *
 * A retained frame exists after a successful sr_render, sr_render_blocks,
 * sr_render_blocks_batch, sr_render_block_list, sr_render_debug,
 * sr_render_phase, sr_render_ss or sr_render_block_list_ss of at least one
 * row. It does not exist before the first launch, after sr_render_adaptive
 * (its sparse sample launch overwrote the plain frame's rays), after
 * sr_render_accumulate or sr_wave_costs, or after a launch of zero rows. A
 * later launch of any kind replaces it.
 *  - sr_set_background keeps it (a reshade reads the current image and size);
 *  - sr_set_texture_array and sr_set_test_ray drop it;
 *  - sr_set_scene keeps it when the new scene differs from the context's
 *    current one in shading-only fields at most (sr_scene_shading_only), and
 *    drops it otherwise; the call itself behaves the same in both cases;
 *  - sr_set_split, sr_set_latency_mode and culling do not matter to it.
 *
 * Shading-only fields, compared as bytes (a NaN equals itself): num_lights
 * and all of lights[]; per material color[0..2], ambient, diffuse, specular,
 * shininess and normal_map_index. Everything else is geometry: objects, every
 * primitive array, planes, materials[].color[3] (opacity), texture_index,
 * invert_uv_x / invert_uv_y / swap_uvs, double_sided_normals, flip_normals,
 * texture_sizes and max_texture_size; a difference there drops the frame even
 * in a material no object uses.
 *
 * Reshade. Definition: sr_reshade writes exactly the bytes the retained call
 * would write if it were issued again now with its own cameras, params and
 * arguments, with the context's current scene, background and texture array.
 * By that definition:
 *  - the rows, layout, batch, block list and the -1 padding and rows past the
 *    frame's end left unwritten are the retained launch's; the pitch and frame
 *    stride are this call's, under the retained call's rules;
 *  - a retained supersampled launch is shaded into the context's sample
 *    scratch and box-resolved into the caller's buffer;
 *  - the retained frame stays valid: reshade any number of times;
 *  - sr_diag_counters()[0] stays 0: a shading-only change cannot turn an
 *    opaque-classified hit translucent.
 * Asynchronous on `stream`, no host wait, ordered like every launch of the
 * context; the geodesics are not walked again (the shade and resume kernels
 * only) and no launch order is learned or touched. */

/* 1 when b differs from a in shading-only fields at most, 0 otherwise (null: 0) */
int sr_scene_shading_only(const sr_scene* a, const sr_scene* b);
/* 1 when the context holds a retained frame that sr_reshade would accept */
int sr_can_reshade(sr_ctx* ctx);

/* SR_E_NOT_READY without a valid retained frame; SR_E_INVALID for a null
 * output, pitch_bytes < 4 * width or, for a batch, frame_stride_bytes <
 * pitch_bytes * rows. Nothing is written in any error case. */
int sr_reshade(sr_ctx* ctx, uint8_t* dev_rgba8, size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);

/* The sr_render_debug form (float FragColor, RGBA8, step counts; dense rows,
 * each may be NULL but not all) of a retained launch of one frame that was
 * not supersampled; SR_E_INVALID otherwise. */
int sr_reshade_debug(sr_ctx* ctx, float* dev_rgba32, uint8_t* dev_rgba8, int32_t* dev_steps, sr_stream stream);

/* Pick. "Which object is under this pixel?" has no straight-ray answer here:
 * light bends, only the retained rays know. Definition: sr_pick_map writes,
 * for every pixel of the retained launch, the code of the first surface on
 * the pixel's ray, in the shader's own walk (frag:930-932; visiting order and
 * strict < as intersect()), that is not a single-sided surface seen from
 * behind (such a surface adds vec4(0) and the ray goes on): the index into
 * scene.objects[], or one of the negative codes below. By that definition:
 *  - a translucent front surface is reported, not what shows through it;
 *  - the flat part of a ray (flat and split modes, radial rays, the tail
 *    beyond 1 / u_f, every escaping ray while the overlay is visible) is the
 *    one unbounded intersect: its closest hit, or SR_PICK_SKY when that is a
 *    back face of a single-sided material (the shader does not look behind);
 *  - the map does not depend on shading-only fields or on reshades in between.
 * One int32 per pixel, rows, layout, batch, block lists and unwritten padding
 * as the retained launch's; dev_ids and pitch_bytes multiples of 4,
 * pitch_bytes >= 4 * width (SR_E_INVALID; for a batch also a stride below
 * pitch_bytes * rows or no multiple of 4). SR_E_NOT_READY without a retained
 * frame and for a retained supersampled launch: the picking surface is the
 * plain frame. Asynchronous on `stream`. */
#define SR_PICK_SKY             (-1)  /* the ray ends in the background */
#define SR_PICK_HOLE            (-2)
#define SR_PICK_TEST_RAY_FLAT   (-3)
#define SR_PICK_TEST_RAY_CURVED (-4)
#define SR_PICK_NONE            (-5)  /* no ray: a pixel the noise mask blacked out */
int sr_pick_map(sr_ctx* ctx, int32_t* dev_ids, size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);

/* ---- Ray maps (not in the reference, whose only output is the colour). What
 * the retained rays know besides a colour and an object code: where on the sky
 * each pixel's bent ray ends (the lens map) and the G-buffer of its first
 * surface, in one cheap pass over the record, without walking a geodesic that
 * already ended.
 *
 * Definition. The maps describe the pixels of the retained launch in the
 * shader's own walk (frag:930-932). "First surface" is exactly sr_pick_map's:
 * a single-sided surface seen from behind is not one.
 *  - id equals sr_pick_map everywhere.
 *  - end is SR_RAY_END_SKY where the pixel's colour ends with a get_bg(dir)
 *    term: rays seen through translucent surfaces, flat rays whose intersect
 *    returned alpha != 1, rays that left the loop by u < 0 or ran out of steps
 *    (frag:935) included; SR_RAY_END_OPAQUE where it ended at a surface whose
 *    shaded alpha is exactly 1 (an object, the hole, a test ray);
 *    SR_RAY_END_NONE where the pixel has no ray (sr_pick_map's SR_PICK_NONE).
 *  - sky_dir and sky_uv are valid where end == SR_RAY_END_SKY: the argument of
 *    that get_bg call and its (u, v) by sr_sky_uv's expressions. Elsewhere they
 *    hold the quiet NaN 0x7fc00000.
 *  - the hit_* maps are valid where id >= 0 and describe that surface; elsewhere
 *    the float maps hold the quiet NaN 0x7fc00000 and hit_step holds -1.
 *    Validity is read from id, never from a NaN: a real value may be NaN under
 *    a non-finite camera.
 *  - hit_step is the value sr_render_debug's step count would have if the ray
 *    ended at that surface: it equals the pixel's step count when hit_base's
 *    alpha is 1, and is 0 in flat mode.
 *  - Deferred shading: where id >= 0, hit_base's alpha is 1 and the crosshair
 *    is off, the pixel's float FragColor rgb is calculate_lighting (frag:406-437)
 *    evaluated on hit_point, hit_normal, hit_view and hit_base with the
 *    object's material terms and the scene's lights, in binary32, in the
 *    shader's order; FragColor.a is 1.
 *  - hit_base, hit_normal and sky_uv follow the context's current scene,
 *    texture array and filter mode, as a reshade does; the rest depends on the
 *    retained rays only.
 * Layout: rows, batch, block list, the -1 padding and the rows past the
 * frame's end left unwritten are the retained launch's, as for sr_pick_map.
 * Element (pixel x, output row k, frame f, component c) of a map with n
 * components is at map[(f * frame_stride_pixels + k * pitch_pixels + x) * n +
 * c]; one pitch, in pixels, serves all maps. Only the maps whose pointer is
 * not NULL are written.
 *
 * The retained frame stays valid, no launch order is learned or touched and
 * sr_diag_counters keeps its meaning. Asynchronous on `stream`, no host wait,
 * ordered like every launch of the context. A pixel whose hit log filled with
 * translucent hits is walked on from its stored state, which is read and not
 * written: a later sr_reshade sees the same record.
 *
 * Nothing is launched or written on a rejection. SR_E_INVALID: a null context
 * or struct, all pointers null, a pointer not 4-byte aligned, pitch_pixels <
 * width or, for a batch, frame_stride_pixels < pitch_pixels * rows.
 * SR_E_NOT_READY: no retained frame, or a retained supersampled launch, as
 * sr_pick_map. */
#define SR_RAY_END_NONE   0  /* no ray: the noise mask, a fisheye pixel beyond PI */
#define SR_RAY_END_SKY    1  /* the pixel's colour ends with a get_bg(dir) term */
#define SR_RAY_END_OPAQUE 2  /* it ended at a surface of alpha exactly 1 (object, hole, test ray) */
typedef struct {
    int32_t* end;        /* 1 per pixel: SR_RAY_END_*                                  */
    int32_t* id;         /* 1: sr_pick_map's code of the first surface                  */
    float*   sky_dir;    /* 3: the argument of the pixel's get_bg call (frag:876/897/905/935) */
    float*   sky_uv;     /* 2: get_bg's (u, v), frag:830-834, under the arithmetic contract  */
    float*   hit_point;  /* 3: hit_info.intersection_point of the first surface         */
    float*   hit_normal; /* 3: `normal` of frag:408-413 (after flip_normals and the normal map) */
    float*   hit_view;   /* 3: view_dir, = -dir of the chord or flat ray that hit       */
    float*   hit_base;   /* 4: base_color of frag:382-405 (rgb albedo, a = the hit's alpha) */
    int32_t* hit_step;   /* 1: geodesic steps the pixel had executed when this surface was found */
} sr_ray_map_ptrs;       /* device pointers, any of them NULL but not all */
int sr_ray_maps(sr_ctx* ctx, const sr_ray_map_ptrs* maps, size_t pitch_pixels,
                size_t frame_stride_pixels, sr_stream stream);
/* Host only, no context: get_bg's (u, v) of a direction, the code the kernel
 * runs (include/sr/sky.hpp): atan2 and asin are the binary64 function rounded
 * to binary32; u = atan2(z, x) / PI, + 2 when negative, * 0.5; v = asin(y) /
 * PI + 0.5. The direction is not normalised. SR_E_INVALID on null arguments. */
int sr_sky_uv(const float dir[3], float out_uv[2]);

/* Split tiles (not in the reference; a latency knob, the pixels are unchanged):
 * the next frames run the max_tiles costliest 16x16 workgroup tiles of the
 * previous frame on this context whose longest ray took at least min_steps
 * steps as waves of lanes_per_wave (16, 4 or 1) rays instead of 64. A wave's
 * budget events are the union of its rays' events, so the frame's longest
 * rays finish sooner in sparse waves, at the cost of more waves for those
 * tiles. max_tiles 0 (the default) turns it off. For one
 * headline frame at a time (1920x1080, 2000 steps) sr_set_split(ctx, 32, 16,
 * 1200) measured 1.148 ms against 1.163 ms without (profiles/r04/s16), and
 * 1.067-1.075 ms against 1.106-1.116 ms timed round robin (profiles/r04/s24). */
int sr_set_split(sr_ctx* ctx, int max_tiles, int lanes_per_wave, int min_steps);

/* Latency mode (not in the reference; the pixels are unchanged): on != 0 runs
 * the next frames' step loop with two fast-loop steps per iteration instead of
 * three: one frame alone finishes sooner (its longest rays' dependency
 * chain: 1.277 -> 1.128 ms in profiles/r04/s8_split_sweep.jsonl), frames in
 * flight run ~2 % slower. For an interactive caller that draws one frame at
 * a time (src/main.cpp:318-319) without split tiles: with them it measured
 * slower than split tiles alone. Off by default. */
int sr_set_latency_mode(sr_ctx* ctx, int on);

/* ---- Projections (not in the reference, whose camera is a pinhole with a
 * field of view below 180 degrees). Context state like sr_set_split and
 * sr_set_latency_mode, but unlike those it changes the pixels: it applies to
 * every later launch of every kind (sr_render, sr_render_blocks,
 * sr_render_blocks_batch, sr_render_block_list, sr_render_ss,
 * sr_render_block_list_ss, sr_render_phase, sr_render_accumulate,
 * sr_render_adaptive, sr_render_debug and sr_wave_costs, whose costs are
 * those of the projected frame).
 *
 * Definition. All arithmetic is binary32 in the order written; sin and cos
 * are the binary64 function of the float argument rounded to binary32
 * (DESIGN.md §4). uv is the pixel's NDC as in every launch (under
 * supersampling and phases the sample frame's), uvv = (uv.x, uv.y * res_y /
 * res_x), a = fov / 360.0f * PI (the shader's own half angle, the argument of
 * the tan behind its forward term), and the local direction L is
 *   RECTILINEAR  (uvv.x, uvv.y, 1 / tan(a)): the reference's pinhole, frag:859-863
 *   EQUIRECT     lon = uvv.x * a, lat = uvv.y * a, cl = cos(lat):
 *                (cl * sin(lon), sin(lat), cl * cos(lon)); longitude and
 *                latitude linear in the pixel, a 2:1 frame at fov 360 is the
 *                whole sphere
 *   FISHEYE      rho = sqrt(uvv.x * uvv.x + uvv.y * uvv.y), th = rho * a; the
 *                pixel has no ray when !(th <= PI) (a NaN has none); else s =
 *                sin(th) and L = rho > 0 ? (s * (uvv.x / rho), s * (uvv.y /
 *                rho), cos(th)) : (0, 0, 1); the equidistant ("angular")
 *                fisheye, a square frame at fov 180 is a dome master
 * and rd = normalize(axes * L) for every projection. Everything after that is
 * the reference's: the radial and flat tests, the split modes on uv, the
 * noise mask on uvv and the crosshair on uv. A pixel with no ray ends exactly
 * like one the noise mask blacked out (the test comes first, before the flat
 * test): FragColor is the crosshair's initial value, it executes 0 steps and
 * sr_pick_map reports SR_PICK_NONE.
 *
 * Setting a different projection drops the retained frame (the retained call
 * issued again would walk other rays); setting the same value keeps it.
 * sr_reshade, sr_reshade_debug and sr_pick_map work after a projected launch
 * as after any other. Launch orders are learned per projection. The call
 * touches host state only: no synchronisation, frames in flight keep the
 * projection they were launched with. Under a projection other than
 * RECTILINEAR the latency mode (sr_set_latency_mode) runs the default unroll;
 * the pixels are the same either way. */
#define SR_PROJECTION_RECTILINEAR 0   /* the reference's pinhole; the default */
#define SR_PROJECTION_EQUIRECT    1   /* longitude / latitude, linear in the pixel */
#define SR_PROJECTION_FISHEYE     2   /* equidistant ("angular") fisheye, dome masters */
/* SR_E_INVALID for a null context or a projection outside 0 .. 2 (nothing changes) */
int sr_set_projection(sr_ctx* ctx, int projection);
/* the context's projection; SR_E_INVALID for a null context */
int sr_get_projection(sr_ctx* ctx);
/* Host only, no context: the local direction L by the rule above of pixel
 * (px, py) of a plain uv_width x uv_height frame (for a supersampled launch:
 * the sample frame's size and the sample's position), the same code the
 * kernel runs. 1: out_local holds the pixel's L; 0: the pixel has no ray
 * (out_local untouched); SR_E_INVALID for an unknown projection, a null
 * output, sizes <= 0 or above INT32_MAX / 2, or a pixel off the frame. */
int sr_projection_dir(int projection, float fov, int uv_width, int uv_height, int px, int py, float out_local[3]);

/* ---- Scene sequences (not in the reference, which uploads its one scene per
 * draw call). The frames of a batched launch (sr_render_blocks_batch,
 * sr_render_block_list) differ only in the camera; an animation in which
 * anything of the scene moves would be a loop of sr_set_scene and sr_render,
 * every frame alone behind a host wait. A sequence holds the animation's
 * scenes on the device, and one launch renders up to 32 frames from
 * consecutive scenes of it, each frame with a camera of its own.
 *
 * Definition. Frame f of a sequence launch holds exactly the bytes sr_render
 * (with ss > 1: sr_render_ss) writes for cams[f] on a context whose scene is
 * scenes[first_scene + f], given the same background, texture array, test
 * ray, projection, params and settings. Layout, pitch, frame stride, the
 * block list's -1 padding and the rows left unwritten are those of
 * sr_render_blocks_batch (one band of rows) and sr_render_block_list(_ss). The
 * launch is asynchronous on `stream` with no host wait, ordered like every
 * launch of the context, and learns and uses the launch order of its grid
 * shape as a batch does.
 *
 * The sequence and the context's own scene (sr_set_scene) are independent
 * states: neither call touches the other's scene or drops the other's
 * retained frame, and a sequence launch does not need sr_set_scene.
 * sr_set_test_ray packs the test-ray part of every scene of the sequence
 * again; sr_set_background, sr_set_texture_array, sr_set_projection,
 * sr_set_split and culling apply to sequence launches as to any launch. The
 * test-ray overlay is tested per chord (as under a projection), and the
 * latency mode (sr_set_latency_mode) runs the default unroll under sequences;
 * the pixels are the same either way. The integrate kernel's slot capacity
 * is chosen per launch for the largest scene of the launch's window.
 *
 * A sequence launch leaves no retained frame ("the context's current scene"
 * has no meaning for it): sr_can_reshade is 0, and sr_reshade,
 * sr_reshade_debug and sr_pick_map return SR_E_NOT_READY until the next plain
 * launch. Sample phases have their sequence form in "Shutter frames" below
 * (sr_render_phase and sr_render_accumulate themselves render the context's
 * own scene); sr_render_adaptive and sr_wave_costs have no sequence form: to
 * price a rank's block lists use sr_set_scene with one scene of the sequence. */
#define SR_MAX_SEQUENCE 256
/* Snapshot copies of n scenes (1 .. SR_MAX_SEQUENCE), each validated and
 * packed as sr_set_scene does with the context's current test ray, uploaded
 * as one array (14,652 bytes per scene). Synchronous like sr_set_scene
 * (waits for the context's frames). Replaces an earlier sequence; n == 0
 * clears it. SR_E_CAPACITY above SR_MAX_SEQUENCE; when scene k is rejected,
 * its status (SR_E_INVALID, SR_E_CAPACITY) and the earlier sequence stays in
 * force. SR_E_INVALID for a null context, n < 0 or null scenes with n > 0. */
int sr_set_scene_sequence(sr_ctx* ctx, const sr_scene* scenes, int n);
/* scenes in the context's sequence (0: none); SR_E_INVALID for a null context */
int sr_scene_sequence_length(sr_ctx* ctx);
/* Rows [row_begin, row_end) of n_frames frames, frame f from scene
 * first_scene + f and cams[f], at dev_rgba8 + f * frame_stride_bytes; ss in
 * 1 .. SR_MAX_SUPERSAMPLE (box-filtered as sr_render_ss). Nothing is launched
 * or written on a rejection: SR_E_NOT_READY without a sequence; SR_E_INVALID
 * when [first_scene, first_scene + n_frames) leaves the sequence;
 * SR_E_CAPACITY above 32 frames; otherwise those of sr_render(_ss) and of
 * sr_render_blocks_batch's frame stride. */
int sr_render_sequence(sr_ctx* ctx, int first_scene, const sr_camera* cams, int n_frames,
                       const sr_params* params, int width, int height, int row_begin, int row_end, int ss,
                       uint8_t* dev_rgba8, size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);
/* The same for the blocks of a list (-1: padding, its rows unwritten), as
 * sr_render_block_list(_ss), whose rejections it adds to the above. */
int sr_render_sequence_block_list(sr_ctx* ctx, int first_scene, const sr_camera* cams, int n_frames,
                                  const sr_params* params, int width, int height, int block_rows,
                                  const int* blocks, int n_blocks, int ss, uint8_t* dev_rgba8,
                                  size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);
/* sr_render_debug of one scene of the sequence: float FragColor, RGBA8 and
 * the executed steps of rows [row_begin, row_end) (any of the three null) */
int sr_render_sequence_debug(sr_ctx* ctx, int scene_index, const sr_camera* cam, const sr_params* params,
                             int width, int height, int row_begin, int row_end, float* dev_rgba32,
                             uint8_t* dev_rgba8, int32_t* dev_steps, sr_stream stream);

/* ---- Shutter frames (not in the reference, whose every frame is an
 * instantaneous snapshot). Time-distributed sampling: output frame m is the
 * mean of K sub-frames, each with its own scene of the sequence, its own
 * camera and its own sub-pixel phase, all M * K of them rendered by ONE
 * batched launch. With K = ss * ss and the progressive phase order, motion
 * blur comes at the price of anti-aliasing alone.
 *
 * Inputs: K = sub_frames >= 1 and M = n_frames >= 1 with M * K <=
 * SR_MAX_BATCH (32); ss in 1 .. SR_MAX_SUPERSAMPLE; cams[M * K]; phases:
 * M * K byte pairs {x, y}, each < ss (host memory, read during the call), or
 * NULL for pair j = sr_phase_order(ss, (j mod K) mod (ss * ss)); first_scene.
 *
 * Definition. Sub-frame j = m * K + k (k < K) is the phase image
 * phase(phases[j]), exactly as "Sample phases" defines it, of the sample
 * frame S_j: the frame this library renders at (ss * width) x (ss * height)
 * for cams[j] with the call's params and the context's textures, test ray,
 * projection and settings. Its scene is scene first_scene + j of the
 * context's sequence, or the context's own scene (sr_set_scene) for every j
 * when first_scene == SR_SHUTTER_OWN_SCENE. Output frame m, every channel
 * alike, in integers:
 *
 *   out_m[y][x][c] = min(255, (sum_{k < K} sub_{m K + k}[y][x][c] + K / 2) div K)
 *
 * which is sr_accum_resolve's rule with n = K. Hence
 *  - K == 1, ss == 1 is sr_render_sequence (own scene: sr_render_blocks_batch)
 *    byte for byte;
 *  - K == ss * ss with one scene, one camera and the default phases is
 *    sr_render_ss byte for byte;
 *  - one scene and one camera with any phases equals sr_render_accumulate and
 *    sr_accum_resolve;
 *  - the crosshair, the noise mask (percent_black) and the split modes
 *    (raytrace_type) are evaluated per sub-frame sample, as in S_j.
 * Layout, pitch, frame stride, the block list's -1 padding and the rows left
 * unwritten are those of sr_render_sequence(_block_list) for M frames; the
 * output pointer, pitch and frame stride must be multiples of 4. The call is
 * asynchronous on `stream` with no host wait. The sub-frames have the grid,
 * the pixel state and the launch order of a plain width x rows batch of M * K
 * frames: the order cached for that shape is learned and used as a batch
 * does; split tiles, culling and the projection apply, and the latency mode
 * as for the underlying launch kind (the default unroll under a sequence).
 * Scratch: the context's sample buffer, 4 * width * rows * M * K bytes, and
 * the pixel state of M * K plain frames (208 bytes per pixel): the memory of
 * M * K plain frames, not of a sample frame per sub-frame.
 *
 * A shutter call leaves no retained frame (sr_can_reshade is 0; sr_reshade,
 * sr_reshade_debug and sr_pick_map return SR_E_NOT_READY until the next plain
 * launch) and touches neither the sequence nor the context's own scene.
 *
 * Rejections, all before anything is launched and with nothing written:
 * SR_E_INVALID for K < 1, M < 1, null pointers, ss out of range, a phase
 * coordinate >= ss, first_scene < -1, a window [first_scene, first_scene +
 * M * K) that leaves the sequence, and the band, pitch, stride, block-list or
 * accumulator errors of sr_render_sequence(_block_list) and
 * sr_render_accumulate; SR_E_CAPACITY for M * K > 32; SR_E_NOT_READY without
 * a sequence, or (own scene) without sr_set_scene; SR_E_NOMEM as for
 * sr_render_accumulate. Shutter forms of sr_render_adaptive, sr_wave_costs,
 * sr_trace_rays and retained frames do not exist; a shutter is a box (every
 * sub-frame weighs the same) over consecutive scenes. */
#define SR_SHUTTER_OWN_SCENE (-1)
/* Rows [row_begin, row_end) of n_frames shutter frames, frame m at dev_rgba8 +
 * m * frame_stride_bytes. */
int sr_render_shutter(sr_ctx* ctx, int first_scene, const sr_camera* cams, const uint8_t* phases, int sub_frames,
                      int n_frames, const sr_params* params, int width, int height, int row_begin, int row_end,
                      int ss, uint8_t* dev_rgba8, size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);
/* The same for the blocks of a list (-1: padding, its rows unwritten): a
 * rank's share in the shape sr_assemble_blocks expects, as
 * sr_render_sequence_block_list. Price the lists with sr_wave_costs on one
 * sub-frame's scene. */
int sr_render_shutter_block_list(sr_ctx* ctx, int first_scene, const sr_camera* cams, const uint8_t* phases,
                                 int sub_frames, int n_frames, const sr_params* params, int width, int height,
                                 int block_rows, const int* blocks, int n_blocks, int ss, uint8_t* dev_rgba8,
                                 size_t pitch_bytes, size_t frame_stride_bytes, sr_stream stream);
/* sr_render_accumulate with a camera and a scene per sub-frame: the n_sub
 * (1 .. 32) sub-frames j of ONE group (cams[j], phases[j] or the default
 * pair of j, scene first_scene + j or the own scene) in one launch, added to
 * the accumulator's rows [0, row_end - row_begin), or stored when reset != 0.
 * Shutters longer than 32 sub-frames (up to SR_MAX_ACCUM_PASSES) take several
 * calls, and any prefix is a displayable frame; resolve with sr_accum_resolve
 * and the number of sub-frames added. Any grouping of a frame's sub-frames
 * resolves to sr_render_shutter's frame, byte for byte. */
int sr_render_accumulate_shutter(sr_ctx* ctx, int first_scene, const sr_camera* cams, const uint8_t* phases,
                                 int n_sub, const sr_params* params, int width, int height, int row_begin,
                                 int row_end, int ss, int reset, uint16_t* dev_accum, size_t accum_pitch_bytes,
                                 sr_stream stream);
/* The group resolve alone, by the rule above: n_frames * sub_frames RGBA8
 * images of width x rows (row r of image j at images + j * image_stride +
 * r * pitch) to n_frames frames, frame m from images m * sub_frames ..
 * (m + 1) * sub_frames - 1, at out + m * out_frame_stride. sub_frames in
 * 1 .. SR_MAX_ACCUM_PASSES, n_frames in 1 .. 65535; pointers, pitches and
 * strides multiples of 4 (multiples of 16 run the kernel's vector path).
 * on_device != 0: device pointers, a kernel on `stream`, asynchronous; 0:
 * host memory, synchronous (the same rule in plain C++). SR_E_INVALID for
 * null pointers, sizes <= 0, a short pitch or stride, a misaligned pointer,
 * pitch or stride, or a count out of range. */
int sr_shutter_resolve(const uint8_t* images, size_t pitch, size_t image_stride, int sub_frames, int n_frames,
                       int width, int rows, uint8_t* out, size_t out_pitch, size_t out_frame_stride, int on_device,
                       sr_stream stream);
/* The default phases (host only): out_pairs[2 k], out_pairs[2 k + 1] =
 * sr_phase_order(ss, k mod (ss * ss)) for k < sub_frames. SR_E_INVALID for ss
 * out of range, sub_frames < 1 or a null pointer. */
int sr_shutter_phases(int ss, int sub_frames, uint8_t* out_pairs);

/* ---- Ray queries (not in the reference, whose every ray starts at the one
 * camera position). A trace launch walks rays the caller supplies, each with
 * an origin of its own: thin-lens depth of field, stereo panoramas, calibrated
 * lens warps, probes inside the scene, line-of-sight tests along bent rays,
 * the press-R test ray on the device.
 *
 * Definition. Ray i of a trace launch has origin O = origins[3 i .. 3 i + 2]
 * and direction V = dirs[3 i .. 3 i + 2]; V need not be normalised. Its
 * results are, bit for bit, those of pixel (0, 0) of a 1 x 1 pinhole
 * (RECTILINEAR) frame of fov 90 whose camera position is O and whose camera
 * axes' columns are (0, 0, V), with crosshair = 0 and percent_black < 0, the
 * context's current scene, test ray, background and texture array, and the
 * call's params. So:
 *   - the direction the walk starts with is normalize((0 * 0 + 0 * 0) + V * 1)
 *     in binary32: normalize(V) with any -0 component of V made +0;
 *   - nv, u, tv and du are the shader's expressions (frag:883-889) on O and
 *     that direction, per ray; the radial test |dot(rd, nv)| >= 1 - 1e-7, the
 *     reseed beyond 1 / u_f, capture, translucency, the test-ray overlay and
 *     the flat tail apply unchanged;
 *   - non-finite or zero O or V, an origin at or inside the horizon or at the
 *     centre are not rejected: they give what the reference's arithmetic gives;
 *   - params->raytrace_type is SR_RAYTRACE_CURVED or SR_RAYTRACE_FLAT (a ray
 *     has no uv: the split modes are SR_E_INVALID); crosshair, percent_black
 *     and curved_percentage are ignored; max_steps, max_revolutions, u_f and
 *     filter_mode are honoured, including the rule that max_revolutions <= 0
 *     or a negative or NaN u_f runs the reference's own loop;
 *   - sr_set_projection, sr_set_split, sr_set_latency_mode and a scene
 *     sequence do not matter to a trace launch; culling applies (never a
 *     result);
 *   - the launch reads and writes no pixel state: a retained frame stays
 *     valid across it (sr_can_reshade, sr_reshade and sr_pick_map see the
 *     last frame launch), learned launch orders stay untouched, and
 *     sr_diag_counters keeps its meaning.
 * A ray's result does not depend on the other rays of the launch or on their
 * order. */
#define SR_TRACE_MAX_RAYS (1 << 28)
/* Inputs: device pointers to n_rays packed xyz triples (12 bytes per ray, 4-byte
 * aligned). Outputs: device pointers, each dense with one entry per ray and
 * 4-byte aligned, any of them NULL but not all: float FragColor (16 bytes per
 * ray); RGBA8 by the frames' conversion (NaN, +inf, -inf store 0, 255, 0);
 * the executed steps; and sr_pick_map's code (an index into scene.objects[]
 * or SR_PICK_*; never SR_PICK_NONE): the first surface on the ray's walk that
 * is not a single-sided surface seen from behind. A launch that asks for
 * dev_ids alone may end each ray at that surface; the ids are the same either
 * way. n_rays == 0: SR_OK, nothing written. Asynchronous on `stream`, no host
 * wait, ordered like every launch of the context. Checked before anything is
 * launched, nothing written: SR_E_INVALID for a null context or params,
 * n_rays < 0 or above SR_TRACE_MAX_RAYS, null or misaligned inputs, misaligned
 * outputs, all outputs NULL, a split mode or unknown raytrace_type or
 * filter_mode, max_steps outside 0 .. SR_MAX_STEPS; SR_E_NOT_READY without a
 * scene. */
int sr_trace_rays(sr_ctx* ctx, const float* dev_origins, const float* dev_dirs, int n_rays,
                  const sr_params* params, float* dev_rgba32, uint8_t* dev_rgba8,
                  int32_t* dev_steps, int32_t* dev_ids, sr_stream stream);
/* Host only, no context: the rays the frame kernels start with, for rows
 * [row_begin, row_end) of a plain width x height frame, row-major from
 * row_begin (3 floats per pixel in each of origins and dirs, host memory).
 * Pixel (px, py): O = the camera's position, V = axes * L in binary32, (c0 *
 * L.x + c1 * L.y) + c2 * L.z with L sr_projection_dir's own; a pixel without
 * a ray (the fisheye beyond PI) gets V = (NaN, NaN, NaN). Traced, these rays
 * give the frame's pixels (where no component of V is -0: see above).
 * SR_E_INVALID for null arguments, an unknown projection, sizes <= 0 or above
 * INT32_MAX / 2, or rows outside 0 <= row_begin <= row_end <= height. */
int sr_camera_rays(const sr_camera* cam, int projection, int width, int height,
                   int row_begin, int row_end, float* origins, float* dirs);

/* ---- Ray maps of ray queries (not in the reference). sr_ray_maps' lens map
 * and G-buffer for rays the caller supplies: where on the sky a probe's ray
 * ends, where in space an arbitrary ray first meets a surface, and with the
 * hit point and normal the start of a second ray (a reflection, an occlusion
 * probe, deferred shading of lens samples).
 *
 * Definition. The maps of ray i are what "Ray maps" gives pixel (0, 0) of the
 * 1 x 1 frame by which "Ray queries" defines ray i: a pinhole of fov 90 with
 * the camera at O and the axes (0, 0, V), crosshair 0, percent_black < 0, the
 * context's current scene, test ray and texture array, and the call's params.
 * So:
 *   - id equals sr_trace_rays' dev_ids for the same rays and params; it is
 *     never SR_PICK_NONE;
 *   - end is SR_RAY_END_SKY or SR_RAY_END_OPAQUE, never SR_RAY_END_NONE:
 *     non-finite or zero O or V are not rejected and give what the
 *     reference's arithmetic gives;
 *   - sky_dir and sky_uv are valid where end == SR_RAY_END_SKY: sky_dir is the
 *     argument of that ray's get_bg call (for a flat ray normalize(+0 + V)),
 *     sky_uv is sr_sky_uv of it. Elsewhere both hold the quiet NaN 0x7fc00000;
 *   - the hit_* maps are valid where id >= 0; elsewhere the float maps hold the
 *     quiet NaN and hit_step holds -1. Validity is read from id, never from a
 *     NaN;
 *   - hit_step is the step count the ray had executed when that surface was
 *     found: sr_trace_rays' dev_steps where hit_base's alpha is 1, and 0 in
 *     flat mode;
 *   - Deferred shading: where id >= 0 and hit_base's alpha is 1, the rgb of
 *     sr_trace_rays' float FragColor of that ray is calculate_lighting
 *     (frag:406-437) on hit_point, hit_normal, hit_view and hit_base, and its
 *     alpha is 1;
 *   - params, context settings and culling are treated as sr_trace_rays treats
 *     them: the split modes are SR_E_INVALID; crosshair, percent_black and
 *     curved_percentage are ignored; max_steps, max_revolutions, u_f and
 *     filter_mode are honoured, with the reference's own loop for
 *     max_revolutions <= 0 or a negative or NaN u_f; culling is never a result;
 *   - no background is needed: the maps look nothing up in it;
 *   - a launch that asks for neither end nor a sky map may end each ray at its
 *     first surface; the other maps are the same either way;
 *   - the launch reads and writes no pixel state and uses no worklist of the
 *     context: a retained frame stays valid across it, learned launch orders
 *     stay untouched and sr_diag_counters keeps its meaning.
 * A ray's maps do not depend on the other rays of the launch or on their order.
 *
 * Layout: dense, one entry per ray: element (ray i, component c) of a map with
 * n components is at map[i * n + c]. Every non-NULL pointer is 4-byte aligned;
 * only the maps whose pointer is not NULL are written, and only their n_rays
 * entries. Inputs as sr_trace_rays'. n_rays == 0: SR_OK, nothing written.
 * Asynchronous on `stream`, no host wait, ordered like every launch of the
 * context. Checked before anything is launched, nothing written: SR_E_INVALID
 * for a null context, params or maps, n_rays < 0 or above SR_TRACE_MAX_RAYS,
 * null or misaligned inputs, all nine pointers NULL or any of them misaligned,
 * a split mode or unknown raytrace_type or filter_mode, max_steps outside
 * 0 .. SR_MAX_STEPS; SR_E_NOT_READY without a scene. */
int sr_trace_ray_maps(sr_ctx* ctx, const float* dev_origins, const float* dev_dirs, int n_rays,
                      const sr_params* params, const sr_ray_map_ptrs* maps, sr_stream stream);

/* Rows a sr_render_blocks call with these arguments writes. */
int sr_blocks_row_count(int height, int block_rows, int block_first, int block_step);

/* Runtime invariant counters of a context (not in the reference), after its
 * launched frames are done: out[0] = pixels the shade kernel found stopped at
 * a hit classified opaque in the step loop whose shaded alpha was not 1 (the
 * classification is exact where it claims, DESIGN.md §5, so this stays 0; a
 * non-zero count means such rays were written without the rest of their
 * path), out[1] = stream-ordered frees (hipFreeAsync) that failed (a leak).
 * Writes min(n, 2) counters. */
int sr_diag_counters(sr_ctx* ctx, int64_t* out, int n);

/* sizeof of the ABI structs, for binding checks: sr_camera, sr_params,
 * sr_scene, sr_test_ray, sr_material, sr_light (in that order). */
int sr_abi_struct_sizes(size_t* out, int n);

/* Presentation (not in the hot path): writes a frame in host memory as an
 * RGBA8 PNG. Replaces the reference's window present (src/main.cpp:318-319
 * draw, :432 glfwSwapBuffers) for offline use. Rows are read bottom-up as GL
 * and sr_render leave them when flip_rows != 0 (row 0 = the image's bottom).
 * SR_E_IO when the file cannot be written. */
int sr_write_png(const char* path, const uint8_t* rgba8, int width, int height, size_t pitch_bytes,
                 int flip_rows);

/* Host-side press-R geodesic (src/main.cpp:94-124): writes up to max_points
 * xyz triples into out_xyz and the count into *out_count. */
int sr_test_ray_points(const float cam_pos[3], const float cam_forward[3], int max_steps,
                       int max_revolutions, float* out_xyz, int max_points, int* out_count);

#ifdef __cplusplus
}
#endif

#endif /* SR_SR_H */
