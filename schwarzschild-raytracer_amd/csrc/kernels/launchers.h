// launchers.h — every extern "C" host entry the kernel files (*.hip) define
// and the C ABI (sr_api.cpp) calls. Included from both sides, so the compiler
// holds each definition to its declaration; a launcher is declared nowhere
// else. The signatures are fixed: tools/build_variant.sh builds an earlier
// revision's geodesic.hip against this tree.
#ifndef SR_KERNELS_LAUNCHERS_H
#define SR_KERNELS_LAUNCHERS_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "device_scene.h"

extern "C" {

// ---- geodesic.hip
hipError_t sr_launch_geodesic(const sr_dev_scene* sc, const float4* tbl, const float* segs, const uint32_t* bg,
                              const uint32_t* arr, const uint8_t* opq, const sr_dev_frame* fr, uint8_t* out,
                              size_t pitch, float* dbg_rgba, int32_t* dbg_steps, float* ps, size_t ps_n, int* list,
                              int* count, int* order, int* cost, int* diag, sr_dev_start* start, hipEvent_t* ev4,
                              hipStream_t stream);
// the frames of a scene sequence (sr.h "Scene sequences"): frame f reads the scene sc[f]; xtab: the scenes'
// low-energy exclusions, 2 * SR_MAX_BUDGET floats each (xlow_need, then xperi_e)
hipError_t sr_launch_geodesic_seq(const sr_dev_scene* sc, const float* xtab, const float4* tbl, const float* segs,
                                  const uint32_t* bg, const uint32_t* arr, const uint8_t* opq, const sr_dev_frame* fr,
                                  uint8_t* out, size_t pitch, float* dbg_rgba, int32_t* dbg_steps, float* ps, size_t ps_n,
                                  int* list, int* count, int* order, int* cost, int* diag, sr_dev_start* start,
                                  hipEvent_t* ev4, hipStream_t stream);
// the shade and resume kernels alone, on pixel state a launch left (sr_reshade)
hipError_t sr_launch_reshade(const sr_dev_scene* sc, const float4* tbl, const float* segs, const uint32_t* bg,
                             const uint32_t* arr, const sr_dev_frame* fr, uint8_t* out, size_t pitch, float* dbg_rgba,
                             int32_t* dbg_steps, float* ps, size_t ps_n, int* list, int* count, int* diag,
                             hipStream_t stream);
// one object code per pixel from that state (sr_pick_map)
hipError_t sr_launch_pick(const sr_dev_scene* sc, const float* segs, const sr_dev_frame* fr, const float* ps,
                          size_t ps_n, int32_t* out, size_t pitch, size_t frame_stride, hipStream_t stream);
// the lens map and the first surface's G-buffer from that state (sr_ray_maps; sr.h "Ray maps"): the requested
// maps (sr.h's struct, device pointers, any of them null), pitch and frame stride in pixels. list / count: the
// context's resume worklist, cleared on the stream here and filled with the pixels whose hit log filled; they are
// walked on by a second kernel (tbl: the step table) when `end` or a sky map is requested. ps is read only.
hipError_t sr_launch_ray_maps(const sr_dev_scene* sc, const float4* tbl, const float* segs, const uint32_t* arr,
                              const sr_dev_frame* fr, const float* ps, size_t ps_n, const sr_ray_map_ptrs* maps,
                              size_t pitch, size_t frame_stride, int* list, int* count, hipStream_t stream);
// caller-supplied rays, one lane each (sr_trace_rays; sr.h "Ray queries"): fr is a 1 x 1 frame's struct with
// win_ok = 0, of which the schedule, the margins, the exclusions and the texture sizes are read; no pixel state
hipError_t sr_launch_trace(const sr_dev_scene* sc, const float4* tbl, const float* segs, const uint32_t* bg,
                           const uint32_t* arr, const sr_dev_frame* fr, const float* origins, const float* dirs,
                           int n_rays, float* out_rgba, uint8_t* out_rgba8, int32_t* out_steps, int32_t* out_ids,
                           hipStream_t stream);
// the lens map and the first surface's G-buffer of caller-supplied rays (sr_trace_ray_maps; sr.h "Ray maps of ray
// queries"): sr_launch_trace's rays and frame, sr_launch_ray_maps' struct of requested maps, dense (one entry per
// ray). No pixel state and no worklist: one kernel walks each ray to its end
hipError_t sr_launch_trace_maps(const sr_dev_scene* sc, const float4* tbl, const float* segs, const uint32_t* arr,
                                const sr_dev_frame* fr, const float* origins, const float* dirs, int n_rays,
                                const sr_ray_map_ptrs* maps, hipStream_t stream);

// ---- assemble.hip
hipError_t sr_assemble_blocks_device(const uint8_t* stacked, size_t rank_stride, size_t in_frame_stride,
                                     const int* dev_lists, int world, int per, int height, int block_rows,
                                     size_t row_bytes, uint8_t* out, size_t out_frame_stride, int n_frames,
                                     hipStream_t stream);
int sr_assemble_blocks_host(const uint8_t* stacked, size_t rank_stride, size_t in_frame_stride, const int* lists,
                            int world, int per, int height, int block_rows, size_t row_bytes, uint8_t* out,
                            size_t out_frame_stride, int n_frames);

// ---- resolve.hip
hipError_t sr_resolve_box_device(const uint8_t* samples, size_t sample_pitch, size_t sample_frame_stride, int width,
                                 int rows, int ss, const int* dev_blocks, int block_rows, int height, uint8_t* out,
                                 size_t pitch, size_t out_frame_stride, int n_frames, hipStream_t stream);
hipError_t sr_resolve_box_masked_device(const uint8_t* samples, size_t sample_pitch, int width, int height, int ss,
                                        const uint8_t* dev_mask, uint8_t* out, size_t pitch, hipStream_t stream);
void sr_resolve_box_host(const uint8_t* samples, size_t sample_pitch, size_t sample_frame_stride, int width, int rows,
                         int ss, uint8_t* out, size_t pitch, size_t out_frame_stride, int n_frames);

// ---- accum.hip
hipError_t sr_accum_add_device(const uint8_t* images, size_t pitch, size_t image_stride, int n_images, int width,
                               int rows, int reset, uint16_t* accum, size_t accum_pitch, hipStream_t stream);
hipError_t sr_accum_resolve_device(const uint16_t* accum, size_t accum_pitch, int width, int rows, int n, uint8_t* out,
                                   size_t pitch, hipStream_t stream);
void sr_accum_add_host(const uint8_t* images, size_t pitch, size_t image_stride, int n_images, int width, int rows,
                       int reset, uint16_t* accum, size_t accum_pitch);
void sr_accum_resolve_host(const uint16_t* accum, size_t accum_pitch, int width, int rows, int n, uint8_t* out,
                           size_t pitch);

// ---- shutter.hip
// the group resolve of sr.h "Shutter frames": n_frames * sub_frames images to n_frames frames
hipError_t sr_shutter_resolve_device(const uint8_t* images, size_t pitch, size_t image_stride, int sub_frames,
                                     int n_frames, int width, int rows, const int* dev_blocks, int block_rows, int height,
                                     uint8_t* out, size_t out_pitch, size_t out_frame_stride, hipStream_t stream);
void sr_shutter_resolve_host(const uint8_t* images, size_t pitch, size_t image_stride, int sub_frames, int n_frames,
                             int width, int rows, uint8_t* out, size_t out_pitch, size_t out_frame_stride);

// ---- adaptive.hip
hipError_t sr_edge_tiles_device(const uint8_t* img, size_t pitch, int width, int height, int threshold, int grow,
                                uint8_t* dev_mask, hipStream_t stream);
hipError_t sr_adaptive_codes_device(const uint8_t* dev_mask, int width, int height, int ss, const int* order,
                                    int n_order, int* codes, uint8_t* user_mask, hipStream_t stream);
void sr_edge_tiles_host(const uint8_t* img, size_t pitch, int width, int height, int threshold, int grow,
                        uint8_t* mask);

}  // extern "C"

#endif
