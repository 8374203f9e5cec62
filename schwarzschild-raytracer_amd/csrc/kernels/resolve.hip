// resolve.hip — box resolve of a supersampled frame (sr.h sr_resolve_box,
// sr_render_ss, sr_render_block_list_ss). Output pixel (x, y), channel c, of
// an ss x ss ordered grid of RGBA8 samples S:
//
//   out[y][x][c] = (sum_{j < ss} sum_{i < ss} S[ss y + j][ss x + i][c] + (ss ss) / 2) div (ss ss)
//
// in integers on the samples' bytes, all four channels alike: the sum does
// not depend on its order, so the kernel, the host form below and numpy on
// the oracle's sample frame give the same bits.
//
// HBM-bound: one lane per output pixel reads ss rows of ss samples, one
// vector load per row (8 B for ss 2, three dwords for ss 3, 16 B for ss 4:
// a wave reads 512 / 768 / 1024 contiguous bytes per sample row) and stores
// one dword. Two channels are summed per 32-bit add (bytes 0, 2 and bytes 1,
// 3 of a sample in 16-bit fields: 16 x 255 fits). A byte path serves sample
// or output addresses that are not aligned for that. One launch covers the
// frames of a batch (blockIdx.y). The kernel knows the block-list layout of
// sr_render_block_list: output slot s holds frame block blocks[s]; a slot
// with -1 and the rows >= height of the frame's last block are skipped,
// their output rows left unwritten and the sample rows behind them never
// read (the launch never wrote them).
//
// Algorithmic bytes = (4 ss^2 + 4) x width x rows per frame (every sample
// read once, every pixel written once).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launchers.h"

namespace {

constexpr int kThreads = 256;

template <int SS>
__device__ __forceinline__ uint32_t box_average(uint32_t even, uint32_t odd) {
    constexpr uint32_t n = SS * SS, half = n / 2;
    const uint32_t c0 = ((even & 0xffffu) + half) / n, c2 = ((even >> 16) + half) / n;
    const uint32_t c1 = ((odd & 0xffffu) + half) / n, c3 = ((odd >> 16) + half) / n;
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

// One output pixel from its ss x ss samples at src (rows sample_pitch apart).
// VEC: the sample rows are aligned for the row's vector load and the output
// for a dword store (checked by the launcher for the whole image).
template <int SS, bool VEC>
__device__ __forceinline__ void resolve_pixel(const uint8_t* __restrict__ src, size_t sample_pitch,
                                              uint8_t* __restrict__ dst) {
    uint32_t even = 0, odd = 0;  // channels 0, 2 and 1, 3 in 16-bit fields
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < SS; j++) {
            const uint8_t* p = src + (size_t)j * sample_pitch;
            uint32_t v[SS];
            if constexpr (SS == 2) {
                const uint2 q = *reinterpret_cast<const uint2*>(p);
                v[0] = q.x, v[1] = q.y;
            } else if constexpr (SS == 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(p);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
                for (int i = 0; i < SS; i++) v[i] = q[i];
            }
#pragma unroll
            for (int i = 0; i < SS; i++) {
                even += v[i] & 0x00ff00ffu;
                odd += (v[i] >> 8) & 0x00ff00ffu;
            }
        }
        *reinterpret_cast<uint32_t*>(dst) = box_average<SS>(even, odd);
    } else {
        for (int j = 0; j < SS; j++) {
            const uint8_t* p = src + (size_t)j * sample_pitch;
            for (int i = 0; i < SS; i++) {
                even += (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 2] << 16);
                odd += (uint32_t)p[4 * i + 1] | ((uint32_t)p[4 * i + 3] << 16);
            }
        }
        const uint32_t v = box_average<SS>(even, odd);
        dst[0] = (uint8_t)v;
        dst[1] = (uint8_t)(v >> 8);
        dst[2] = (uint8_t)(v >> 16);
        dst[3] = (uint8_t)(v >> 24);
    }
}

template <int SS, bool VEC>
__global__ __launch_bounds__(kThreads) void sr_resolve_kernel(const uint8_t* __restrict__ samples, size_t sample_pitch,
                                                              size_t sample_frame_stride, int width, int x_chunks,
                                                              const int* __restrict__ blocks, int block_rows, int height,
                                                              uint8_t* __restrict__ out, size_t pitch,
                                                              size_t out_frame_stride) {
    const int row = blockIdx.x / x_chunks;  // output row of the tile
    const int x = (blockIdx.x % x_chunks) * kThreads + threadIdx.x;
    if (blocks) {
        const int b = blocks[row / block_rows];
        if (b < 0 || b * block_rows + row % block_rows >= height) return;
    }
    if (x >= width) return;
    const uint8_t* src = samples + (size_t)blockIdx.y * sample_frame_stride + (size_t)row * SS * sample_pitch +
                         (size_t)x * (4 * SS);
    uint8_t* dst = out + (size_t)blockIdx.y * out_frame_stride + (size_t)row * pitch + (size_t)x * 4;
    resolve_pixel<SS, VEC>(src, sample_pitch, dst);
}

// The masked resolve of sr_render_adaptive (adaptive.hip): one workgroup per
// 16x16 output tile, lane t its pixel (t % 16, t / 16). Only the tiles with
// mask[tile] != 0 are resolved, clipped to the frame: the sparse sample launch
// wrote exactly their samples, so no other scratch is read, and the other
// tiles of `out` keep the plain frame.
template <int SS, bool VEC>
__global__ __launch_bounds__(kThreads) void sr_resolve_masked_kernel(const uint8_t* __restrict__ samples,
                                                                     size_t sample_pitch, int width, int height, int gx,
                                                                     const uint8_t* __restrict__ mask,
                                                                     uint8_t* __restrict__ out, size_t pitch) {
    const int tile = blockIdx.x;
    if (!mask[tile]) return;
    const int x = (tile % gx) * 16 + (int)(threadIdx.x & 15), y = (tile / gx) * 16 + (int)(threadIdx.x >> 4);
    if (x >= width || y >= height) return;
    resolve_pixel<SS, VEC>(samples + (size_t)y * SS * sample_pitch + (size_t)x * (4 * SS), sample_pitch,
                           out + (size_t)y * pitch + (size_t)x * 4);
}

template <int SS>
hipError_t launch_resolve_masked(const uint8_t* samples, size_t sample_pitch, int width, int height,
                                 const uint8_t* dev_mask, uint8_t* out, size_t pitch, hipStream_t stream) {
    const int gx = (width + 15) / 16, gy = (height + 15) / 16;
    if ((long long)gx * gy > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t load = SS == 3 ? 4 : 4 * SS;
    const bool vec = (((uintptr_t)samples | sample_pitch) & (load - 1)) == 0 && (((uintptr_t)out | pitch) & 3) == 0;
    const dim3 grid((unsigned)(gx * gy));
    if (vec)
        hipLaunchKernelGGL((sr_resolve_masked_kernel<SS, true>), grid, dim3(kThreads), 0, stream, samples, sample_pitch,
                           width, height, gx, dev_mask, out, pitch);
    else
        hipLaunchKernelGGL((sr_resolve_masked_kernel<SS, false>), grid, dim3(kThreads), 0, stream, samples,
                           sample_pitch, width, height, gx, dev_mask, out, pitch);
    return hipGetLastError();
}

template <int SS>
hipError_t launch_resolve(const uint8_t* samples, size_t sample_pitch, size_t sample_frame_stride, int width, int rows,
                          const int* dev_blocks, int block_rows, int height, uint8_t* out, size_t pitch,
                          size_t out_frame_stride, int n_frames, hipStream_t stream) {
    const int x_chunks = (width + kThreads - 1) / kThreads;
    if ((long long)x_chunks * rows > 0x7fffffffLL || n_frames > 65535) return hipErrorInvalidValue;
    const size_t load = SS == 3 ? 4 : 4 * SS;
    const bool vec = (((uintptr_t)samples | sample_pitch | sample_frame_stride) & (load - 1)) == 0 &&
                     (((uintptr_t)out | pitch | out_frame_stride) & 3) == 0;
    const dim3 grid((unsigned)(x_chunks * rows), (unsigned)n_frames);
    if (vec)
        hipLaunchKernelGGL((sr_resolve_kernel<SS, true>), grid, dim3(kThreads), 0, stream, samples, sample_pitch,
                           sample_frame_stride, width, x_chunks, dev_blocks, block_rows, height, out, pitch,
                           out_frame_stride);
    else
        hipLaunchKernelGGL((sr_resolve_kernel<SS, false>), grid, dim3(kThreads), 0, stream, samples, sample_pitch,
                           sample_frame_stride, width, x_chunks, dev_blocks, block_rows, height, out, pitch,
                           out_frame_stride);
    return hipGetLastError();
}

}  // namespace

// n_frames tiles of `rows` output rows from dense sample tiles of ss x rows
// rows. dev_blocks != nullptr: the tile is a block list's (rows = its slots x
// block_rows, block_rows and height in output rows); nullptr: every row.
extern "C" hipError_t sr_resolve_box_device(const uint8_t* samples, size_t sample_pitch, size_t sample_frame_stride,
                                            int width, int rows, int ss, const int* dev_blocks, int block_rows,
                                            int height, uint8_t* out, size_t pitch, size_t out_frame_stride,
                                            int n_frames, hipStream_t stream) {
    if (width <= 0 || rows <= 0 || n_frames <= 0) return hipSuccess;
    if (dev_blocks && block_rows <= 0) return hipErrorInvalidValue;
    switch (ss) {
    case 1:
        return launch_resolve<1>(samples, sample_pitch, sample_frame_stride, width, rows, dev_blocks, block_rows, height,
                                 out, pitch, out_frame_stride, n_frames, stream);
    case 2:
        return launch_resolve<2>(samples, sample_pitch, sample_frame_stride, width, rows, dev_blocks, block_rows, height,
                                 out, pitch, out_frame_stride, n_frames, stream);
    case 3:
        return launch_resolve<3>(samples, sample_pitch, sample_frame_stride, width, rows, dev_blocks, block_rows, height,
                                 out, pitch, out_frame_stride, n_frames, stream);
    case 4:
        return launch_resolve<4>(samples, sample_pitch, sample_frame_stride, width, rows, dev_blocks, block_rows, height,
                                 out, pitch, out_frame_stride, n_frames, stream);
    default:
        return hipErrorInvalidValue;
    }
}

// The flagged 16x16 tiles (dev_mask[ceil(height / 16)][ceil(width / 16)], bytes
// 0 / 1) of a whole width x height frame from its full-size sample frame.
extern "C" hipError_t sr_resolve_box_masked_device(const uint8_t* samples, size_t sample_pitch, int width, int height,
                                                   int ss, const uint8_t* dev_mask, uint8_t* out, size_t pitch,
                                                   hipStream_t stream) {
    if (width <= 0 || height <= 0) return hipSuccess;
    switch (ss) {
    case 2: return launch_resolve_masked<2>(samples, sample_pitch, width, height, dev_mask, out, pitch, stream);
    case 3: return launch_resolve_masked<3>(samples, sample_pitch, width, height, dev_mask, out, pitch, stream);
    case 4: return launch_resolve_masked<4>(samples, sample_pitch, width, height, dev_mask, out, pitch, stream);
    default: return hipErrorInvalidValue;
    }
}

// The same rule in plain C++ on host memory.
extern "C" void sr_resolve_box_host(const uint8_t* samples, size_t sample_pitch, size_t sample_frame_stride, int width,
                                    int rows, int ss, uint8_t* out, size_t pitch, size_t out_frame_stride,
                                    int n_frames) {
    const unsigned n = (unsigned)(ss * ss), half = n / 2;
    for (int f = 0; f < n_frames; f++)
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < width; x++) {
                unsigned sum[4] = {0, 0, 0, 0};
                for (int j = 0; j < ss; j++) {
                    const uint8_t* p = samples + (size_t)f * sample_frame_stride +
                                       ((size_t)y * ss + j) * sample_pitch + (size_t)x * ss * 4;
                    for (int i = 0; i < ss; i++)
                        for (int c = 0; c < 4; c++) sum[c] += p[4 * i + c];
                }
                uint8_t* d = out + (size_t)f * out_frame_stride + (size_t)y * pitch + (size_t)x * 4;
                for (int c = 0; c < 4; c++) d[c] = (uint8_t)((sum[c] + half) / n);
            }
}
