// accum.hip — the 16-bit accumulator of progressive supersampling (sr.h
// sr_accum_add, sr_accum_resolve, sr_render_accumulate). An accumulator is
// uint16_t[rows][width][4] with a pitch in bytes; RGBA8 images are added to it
// channel by channel in plain 16-bit adds (modulo 2^16) and resolved by
//
//   out[y][x][c] = min(255, (acc[y][x][c] + n / 2) div n)
//
// in integers, n in 1 .. SR_MAX_ACCUM_PASSES (256 x 255 fits 16 bits). A sum
// does not depend on its order or grouping, so the kernels, the host forms
// below and numpy give the same bits.
//
// HBM-bound, one lane per output pixel. The add reads the pixel's dword from
// each of the n images (a wave reads 256 contiguous bytes per image row),
// sums two channels per 32-bit add (bytes 0, 2 and bytes 1, 3 in 16-bit
// fields, as resolve.hip does: 256 x 255 fits) and does one 8-byte
// read-modify-write of the accumulator (a plain store when reset is set: the
// accumulator is never read). The resolve is one 8-byte load and one dword
// store. Algorithmic bytes per pixel: 4 n + 16 (8 with reset) and 12.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launchers.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void sr_accum_add_kernel(const uint8_t* __restrict__ images, size_t pitch,
                                                                size_t image_stride, int n_images, int width,
                                                                int x_chunks, int reset, uint8_t* __restrict__ accum,
                                                                size_t accum_pitch) {
    const int row = blockIdx.x / x_chunks;
    const int x = (blockIdx.x % x_chunks) * kThreads + threadIdx.x;
    if (x >= width) return;
    const uint8_t* src = images + (size_t)row * pitch + (size_t)x * 4;
    uint32_t even = 0, odd = 0;  // channels 0, 2 and 1, 3 in 16-bit fields
    for (int k = 0; k < n_images; k++) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (size_t)k * image_stride);
        even += v & 0x00ff00ffu;
        odd += (v >> 8) & 0x00ff00ffu;
    }
    // the accumulator's dwords: channels 0, 1 and 2, 3
    uint2 a = make_uint2((even & 0xffffu) | (odd << 16), (even >> 16) | (odd & 0xffff0000u));
    uint2* dst = reinterpret_cast<uint2*>(accum + (size_t)row * accum_pitch + (size_t)x * 8);
    if (!reset) {
        const uint2 b = *dst;  // each field modulo 2^16: no carry from the low field into the high one
        a.x = ((a.x + b.x) & 0xffffu) | ((a.x & 0xffff0000u) + (b.x & 0xffff0000u));
        a.y = ((a.y + b.y) & 0xffffu) | ((a.y & 0xffff0000u) + (b.y & 0xffff0000u));
    }
    *dst = a;
}

// (acc + n / 2) div n for acc <= 65535, n <= 256: 32-bit integer division,
// exact for every operand
__device__ __forceinline__ uint32_t resolve_channel(uint32_t acc, uint32_t n, uint32_t half) {
    const uint32_t q = (acc + half) / n;
    return q < 255u ? q : 255u;
}

__global__ __launch_bounds__(kThreads) void sr_accum_resolve_kernel(const uint8_t* __restrict__ accum,
                                                                    size_t accum_pitch, int width, int x_chunks,
                                                                    uint32_t n, uint8_t* __restrict__ out,
                                                                    size_t pitch) {
    const int row = blockIdx.x / x_chunks;
    const int x = (blockIdx.x % x_chunks) * kThreads + threadIdx.x;
    if (x >= width) return;
    const uint2 a = *reinterpret_cast<const uint2*>(accum + (size_t)row * accum_pitch + (size_t)x * 8);
    const uint32_t half = n / 2;
    const uint32_t c0 = resolve_channel(a.x & 0xffffu, n, half), c1 = resolve_channel(a.x >> 16, n, half);
    const uint32_t c2 = resolve_channel(a.y & 0xffffu, n, half), c3 = resolve_channel(a.y >> 16, n, half);
    *reinterpret_cast<uint32_t*>(out + (size_t)row * pitch + (size_t)x * 4) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

}  // namespace

// Every argument was checked by the caller (sr_api.cpp): dword-aligned
// images and output, an 8-byte-aligned accumulator, pitches that hold a row.
extern "C" hipError_t sr_accum_add_device(const uint8_t* images, size_t pitch, size_t image_stride, int n_images,
                                          int width, int rows, int reset, uint16_t* accum, size_t accum_pitch,
                                          hipStream_t stream) {
    if (width <= 0 || rows <= 0) return hipSuccess;
    const int x_chunks = (width + kThreads - 1) / kThreads;
    if ((long long)x_chunks * rows > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sr_accum_add_kernel, dim3((unsigned)(x_chunks * rows)), dim3(kThreads), 0, stream, images, pitch,
                       image_stride, n_images, width, x_chunks, reset, reinterpret_cast<uint8_t*>(accum), accum_pitch);
    return hipGetLastError();
}

extern "C" hipError_t sr_accum_resolve_device(const uint16_t* accum, size_t accum_pitch, int width, int rows, int n,
                                              uint8_t* out, size_t pitch, hipStream_t stream) {
    if (width <= 0 || rows <= 0) return hipSuccess;
    const int x_chunks = (width + kThreads - 1) / kThreads;
    if ((long long)x_chunks * rows > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sr_accum_resolve_kernel, dim3((unsigned)(x_chunks * rows)), dim3(kThreads), 0, stream,
                       reinterpret_cast<const uint8_t*>(accum), accum_pitch, width, x_chunks, (uint32_t)n, out, pitch);
    return hipGetLastError();
}

// The same rules in plain C++ on host memory.
extern "C" void sr_accum_add_host(const uint8_t* images, size_t pitch, size_t image_stride, int n_images, int width,
                                  int rows, int reset, uint16_t* accum, size_t accum_pitch) {
    for (int y = 0; y < rows; y++) {
        uint16_t* a = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(accum) + (size_t)y * accum_pitch);
        for (int x = 0; x < width; x++)
            for (int c = 0; c < 4; c++) {
                unsigned sum = reset ? 0u : a[4 * x + c];
                for (int k = 0; k < n_images; k++) sum += images[(size_t)k * image_stride + (size_t)y * pitch + 4 * x + c];
                a[4 * x + c] = (uint16_t)sum;
            }
    }
}

extern "C" void sr_accum_resolve_host(const uint16_t* accum, size_t accum_pitch, int width, int rows, int n,
                                      uint8_t* out, size_t pitch) {
    const unsigned un = (unsigned)n, half = un / 2;
    for (int y = 0; y < rows; y++) {
        const uint16_t* a =
            reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(accum) + (size_t)y * accum_pitch);
        uint8_t* d = out + (size_t)y * pitch;
        for (int x = 0; x < 4 * width; x++) {
            const unsigned q = ((unsigned)a[x] + half) / un;
            d[x] = (uint8_t)(q < 255u ? q : 255u);
        }
    }
}
