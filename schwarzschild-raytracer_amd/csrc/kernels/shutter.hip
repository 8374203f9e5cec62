// shutter.hip — the group resolve of shutter frames (sr.h "Shutter frames":
// sr_render_shutter, sr_render_shutter_block_list, sr_shutter_resolve). Output
// frame m, pixel (x, y), channel c, of K sub-frame images I_{mK} .. I_{mK+K-1}
// (RGBA8, image j at images + j * image_stride):
//
//   out_m[y][x][c] = min(255, (sum_{k < K} I_{mK+k}[y][x][c] + K / 2) div K)
//
// in integers on the images' bytes, all four channels alike, K in 1 ..
// SR_MAX_ACCUM_PASSES: sr_accum_resolve's rule with n = K, without the 16-bit
// accumulator in between. The sum does not depend on its order, so the kernel,
// the host form below and numpy give the same bits.
//
// HBM-bound: every image byte is read once and every output byte written
// once, 4 K + 4 algorithmic bytes per pixel. Two channels are summed per
// 32-bit add (bytes 0, 2 and bytes 1, 3 of a pixel in 16-bit fields, as
// accum.hip and resolve.hip do: 256 x 255 + 128 fits). The vector path gives a
// lane four adjacent pixels: one 16-byte load per image (a wave reads 1 KiB
// of an image row per instruction) and one 16-byte store; it needs every
// pointer, pitch and stride to be a multiple of 16, and a row's last one to
// three pixels go through the dword form. The dword path (one pixel per
// lane) serves buffers aligned to 4 only. K is a run-time value: the division
// is shutter_div.h's multiplication, exact for every operand. One launch
// covers the M frames (blockIdx.y). The kernel knows the block-list layout
// of sr_render_block_list as sr_resolve_kernel does: output slot s holds
// frame block blocks[s]; a slot with -1 and the rows >= height of the frame's
// last block are skipped, their output rows left unwritten and the image
// rows behind them never read (the launch never wrote them).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launchers.h"
#include "shutter_div.h"

namespace {

constexpr int kThreads = 256;

// the rule on one pixel's sums: channels 0, 2 in `even` and 1, 3 in `odd` (16-bit fields)
__device__ __forceinline__ uint32_t shutter_average(uint32_t even, uint32_t odd, uint32_t half, uint32_t magic) {
    const uint32_t c0 = sr_shutter_div((even & 0xffffu) + half, magic), c2 = sr_shutter_div((even >> 16) + half, magic);
    const uint32_t c1 = sr_shutter_div((odd & 0xffffu) + half, magic), c3 = sr_shutter_div((odd >> 16) + half, magic);
    // K sums of at most 255 each: the quotient is at most 255 (the definition's min never binds)
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

__device__ __forceinline__ uint32_t shutter_pixel(const uint8_t* __restrict__ src, size_t image_stride, int k_images,
                                                  uint32_t half, uint32_t magic) {
    uint32_t even = 0, odd = 0;
    for (int k = 0; k < k_images; k++) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (size_t)k * image_stride);
        even += v & 0x00ff00ffu;
        odd += (v >> 8) & 0x00ff00ffu;
    }
    return shutter_average(even, odd, half, magic);
}

// VEC: four pixels per lane (x_chunks counts chunks of 4 * kThreads pixels), else one
template <bool VEC>
__global__ __launch_bounds__(kThreads) void sr_shutter_resolve_kernel(const uint8_t* __restrict__ images, size_t pitch,
                                                                      size_t image_stride, int k_images, uint32_t magic,
                                                                      int width, int x_chunks,
                                                                      const int* __restrict__ blocks, int block_rows,
                                                                      int height, uint8_t* __restrict__ out,
                                                                      size_t out_pitch, size_t out_frame_stride) {
    const int row = blockIdx.x / x_chunks;  // output row of the tile
    const int x = ((blockIdx.x % x_chunks) * kThreads + threadIdx.x) * (VEC ? 4 : 1);
    if (blocks) {
        const int b = blocks[row / block_rows];
        if (b < 0 || b * block_rows + row % block_rows >= height) return;
    }
    if (x >= width) return;
    const uint32_t half = (uint32_t)k_images / 2;
    // frame m's first image is image m K
    const uint8_t* src = images + (size_t)blockIdx.y * (size_t)k_images * image_stride + (size_t)row * pitch + (size_t)x * 4;
    uint8_t* dst = out + (size_t)blockIdx.y * out_frame_stride + (size_t)row * out_pitch + (size_t)x * 4;
    if constexpr (VEC) {
        if (x + 4 <= width) {
            uint32_t even[4] = {0, 0, 0, 0}, odd[4] = {0, 0, 0, 0};
#pragma unroll 4
            for (int k = 0; k < k_images; k++) {
                const uint4 q = *reinterpret_cast<const uint4*>(src + (size_t)k * image_stride);
                const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    even[i] += v[i] & 0x00ff00ffu;
                    odd[i] += (v[i] >> 8) & 0x00ff00ffu;
                }
            }
            *reinterpret_cast<uint4*>(dst) =
                make_uint4(shutter_average(even[0], odd[0], half, magic), shutter_average(even[1], odd[1], half, magic),
                           shutter_average(even[2], odd[2], half, magic), shutter_average(even[3], odd[3], half, magic));
            return;
        }
        for (int i = 0; x + i < width; i++)  // the row's last pixels: no load or store past the row
            *reinterpret_cast<uint32_t*>(dst + 4 * i) = shutter_pixel(src + 4 * i, image_stride, k_images, half, magic);
    } else {
        *reinterpret_cast<uint32_t*>(dst) = shutter_pixel(src, image_stride, k_images, half, magic);
    }
}

}  // namespace

// n_frames tiles of `rows` output rows from n_frames * sub_frames image tiles
// of the same shape. dev_blocks != nullptr: the tiles are a block list's (rows
// = its slots x block_rows); nullptr: every row. Every argument was checked by
// the caller (sr_api.cpp): dword-aligned pointers, pitches and strides,
// pitches that hold a row, sub_frames in 1 .. 256.
extern "C" hipError_t sr_shutter_resolve_device(const uint8_t* images, size_t pitch, size_t image_stride, int sub_frames,
                                                int n_frames, int width, int rows, const int* dev_blocks, int block_rows,
                                                int height, uint8_t* out, size_t out_pitch, size_t out_frame_stride,
                                                hipStream_t stream) {
    if (width <= 0 || rows <= 0 || n_frames <= 0) return hipSuccess;
    if (sub_frames < 1 || sub_frames > 256 || n_frames > 65535) return hipErrorInvalidValue;
    if (dev_blocks && block_rows <= 0) return hipErrorInvalidValue;
    const bool vec = (((uintptr_t)images | pitch | image_stride | (uintptr_t)out | out_pitch | out_frame_stride) & 15) == 0;
    const int per_lane = vec ? 4 : 1;
    const int x_chunks = (int)(((long long)width + (long long)kThreads * per_lane - 1) / ((long long)kThreads * per_lane));
    if ((long long)x_chunks * rows > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(x_chunks * rows), (unsigned)n_frames);
    const uint32_t magic = sr_shutter_magic((uint32_t)sub_frames);
    if (vec)
        hipLaunchKernelGGL(sr_shutter_resolve_kernel<true>, grid, dim3(kThreads), 0, stream, images, pitch, image_stride,
                           sub_frames, magic, width, x_chunks, dev_blocks, block_rows, height, out, out_pitch,
                           out_frame_stride);
    else
        hipLaunchKernelGGL(sr_shutter_resolve_kernel<false>, grid, dim3(kThreads), 0, stream, images, pitch, image_stride,
                           sub_frames, magic, width, x_chunks, dev_blocks, block_rows, height, out, out_pitch,
                           out_frame_stride);
    return hipGetLastError();
}

// The same rule in plain C++ on host memory.
extern "C" void sr_shutter_resolve_host(const uint8_t* images, size_t pitch, size_t image_stride, int sub_frames,
                                        int n_frames, int width, int rows, uint8_t* out, size_t out_pitch,
                                        size_t out_frame_stride) {
    const unsigned n = (unsigned)sub_frames, half = n / 2;
    for (int m = 0; m < n_frames; m++)
        for (int y = 0; y < rows; y++) {
            uint8_t* d = out + (size_t)m * out_frame_stride + (size_t)y * out_pitch;
            for (int x = 0; x < 4 * width; x++) {
                unsigned sum = 0;
                for (int k = 0; k < sub_frames; k++)
                    sum += images[((size_t)m * sub_frames + k) * image_stride + (size_t)y * pitch + x];
                const unsigned q = (sum + half) / n;
                d[x] = (uint8_t)(q < 255u ? q : 255u);
            }
        }
}
