// adaptive.hip — tile selection of adaptive supersampling (sr.h
// sr_render_adaptive, sr_edge_tiles): which 16x16 output tiles of the plain
// frame P hold an edge, and the launch codes of the sample frame's tiles
// behind them.
//
// Edge rule, on P's RGBA8 bytes, all four channels alike: two pixels that are
// horizontal or vertical neighbours inside the frame form an edge pair when
// max_c |a_c - b_c| > threshold. A tile is seeded when a pixel of it belongs
// to an edge pair (a pair that straddles a tile boundary seeds both tiles);
// threshold < 0 seeds every tile, threshold >= 255 none. The flagged set is
// the seeded set dilated `grow` times by the 3x3 neighbourhood on the tile
// grid, which is the seeded set's Chebyshev neighbourhood of radius `grow`.
//
// Selection: one 256-thread workgroup per output tile. It stages the tile's
// pixels with a one-pixel halo in LDS (18 x 18 dwords), every lane compares
// its pixel with its in-frame neighbours, those across the tile's border
// included (the rule is symmetric, so a straddling pair seeds both tiles
// without atomics), and one workgroup-wide OR gives the seed. A seeded tile
// writes 1 to the mask entries within `grow` of it: the mask is cleared on
// the stream ahead of the kernel, concurrent stores all store 1, and the
// dilation needs no second pass and no scratch.
//
// Codes: a flagged tile (tx, ty) is exactly the ss x ss block of the sample
// frame's own 16x16 workgroup tiles (ss tx + i, ss ty + j); the ones past the
// sample grid's edge on a partial tile do not exist. Their launch codes
// (tile << 8, geodesic.hip) are compacted to the front of the code list; the
// list was filled with -1 ("exit") on the stream ahead of the kernel. The
// order of the codes is free for the pixels (a ray's result does not depend
// on which rays share its wave) but not for the time: they follow the plain
// frame's own launch order, costliest tiles first.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launchers.h"

namespace {

constexpr int kThreads = 256;
constexpr int kHalo = 18;  // 16 + a pixel on each side

// max over the four channels of |a_c - b_c|
__host__ __device__ inline int channel_distance(uint32_t a, uint32_t b) {
    int m = 0;
    for (int c = 0; c < 4; c++) {
        const int d = (int)((a >> (8 * c)) & 0xffu) - (int)((b >> (8 * c)) & 0xffu);
        m = d < 0 ? (-d > m ? -d : m) : (d > m ? d : m);
    }
    return m;
}

__host__ __device__ inline uint32_t load_pixel(const uint8_t* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// `mask` ([gy][gx] bytes) was cleared ahead of this kernel.
__global__ __launch_bounds__(kThreads) void sr_edge_seed_kernel(const uint8_t* __restrict__ img, size_t pitch, int width,
                                                                int height, int gx, int gy, int threshold, int grow,
                                                                int aligned, uint8_t* __restrict__ mask) {
    __shared__ uint32_t px[kHalo][kHalo];
    const int tx = (int)blockIdx.x % gx, ty = (int)blockIdx.x / gx;
    const int x0 = tx * 16 - 1, y0 = ty * 16 - 1;  // the halo's corner
    int edge = threshold < 0;
    if (!edge) {  // (workgroup-uniform)
        for (int k = threadIdx.x; k < kHalo * kHalo; k += kThreads) {
            const int lx = k % kHalo, ly = k / kHalo;
            const int x = x0 + lx, y = y0 + ly;
            uint32_t v = 0;
            if (x >= 0 && x < width && y >= 0 && y < height)
                v = load_pixel(img + (size_t)y * pitch + (size_t)x * 4, aligned != 0);
            px[ly][lx] = v;
        }
        __syncthreads();
        const int lx = (int)(threadIdx.x & 15) + 1, ly = (int)(threadIdx.x >> 4) + 1;
        const int x = x0 + lx, y = y0 + ly;
        if (x < width && y < height) {
            const uint32_t a = px[ly][lx];
            int d = 0;
            if (x > 0) d = max(d, channel_distance(a, px[ly][lx - 1]));
            if (x + 1 < width) d = max(d, channel_distance(a, px[ly][lx + 1]));
            if (y > 0) d = max(d, channel_distance(a, px[ly - 1][lx]));
            if (y + 1 < height) d = max(d, channel_distance(a, px[ly + 1][lx]));
            edge = d > threshold;
        }
    }
    if (__syncthreads_or(edge)) {
        const int side = 2 * grow + 1;
        if ((int)threadIdx.x < side * side) {
            const int nx = tx + (int)threadIdx.x % side - grow, ny = ty + (int)threadIdx.x / side - grow;
            if (nx >= 0 && nx < gx && ny >= 0 && ny < gy) mask[(size_t)ny * gx + nx] = 1;
        }
    }
}

// One workgroup. `order` is the plain frame's launch order (geodesic.hip
// order_tiles: its n_order codes name every output tile once, costliest
// first, as tile << 8 or as the workgroups tile << 8 | SR_SPLIT | sub of a
// split tile; -1 = unused slot), written by the plain frame's shade kernel
// just before on the same stream. The flagged tiles' sample tiles are emitted
// in that order by a running prefix sum over chunks of the list, so the
// sample launch starts its long rays first as a learned order would; the
// rest of codes[0 .. sgx * sgy) was filled with -1 ahead of this kernel.
constexpr int kCodesThreads = 1024;
constexpr int kSplit = 0x80;  // geodesic.hip SR_SPLIT

__global__ __launch_bounds__(kCodesThreads) void sr_adaptive_codes_kernel(const uint8_t* __restrict__ mask, int tiles,
                                                                          int gx, int ss, int sgx, int sgy,
                                                                          const int* __restrict__ order, int n_order,
                                                                          int* __restrict__ codes,
                                                                          uint8_t* __restrict__ user_mask) {
    __shared__ int wsum[kCodesThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (user_mask)
        for (int i = t; i < tiles; i += kCodesThreads) user_mask[i] = mask[i];
    const int stiles = sgx * sgy;
    int base = 0;  // codes emitted by the chunks before this one (the same in every thread)
    for (int first = 0; first < n_order; first += kCodesThreads) {
        const int slot = first + t;
        const int code = slot < n_order ? order[slot] : -1;
        const int tile = code >> 8;
        // a split tile counts once, at its first workgroup
        const bool take = code >= 0 && (!(code & kSplit) || (code & 0x3f) == 0) && tile < tiles && mask[tile] != 0;
        int sx0 = 0, sy0 = 0, nx = 0, ny = 0;
        if (take) {
            sx0 = (tile % gx) * ss, sy0 = (tile / gx) * ss;  // < sgx, < sgy: the tile holds a pixel of the frame
            nx = min(ss, sgx - sx0), ny = min(ss, sgy - sy0);
        }
        const int n = nx * ny;
        int x = n;  // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kCodesThreads / 64; k++) {
            before += k < wv ? wsum[k] : 0;
            total += wsum[k];
        }
        int at = base + before + x - n;
        if (at + n <= stiles)  // (every tile is listed once, so this holds)
            for (int j = 0; j < ny; j++)
                for (int i = 0; i < nx; i++) codes[at++] = ((sy0 + j) * sgx + sx0 + i) << 8;
        base += total;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
}

}  // namespace

// The flagged set of a width x height RGBA8 image in device memory into
// dev_mask[ceil(height / 16)][ceil(width / 16)] (bytes 0 / 1), on `stream`.
extern "C" hipError_t sr_edge_tiles_device(const uint8_t* img, size_t pitch, int width, int height, int threshold,
                                           int grow, uint8_t* dev_mask, hipStream_t stream) {
    const int gx = (width + 15) / 16, gy = (height + 15) / 16;
    if (width <= 0 || height <= 0 || grow < 0 || grow > 2 || (long long)gx * gy > 0x7fffffffLL)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(dev_mask, 0, (size_t)gx * gy, stream);
    if (e != hipSuccess) return e;
    if (threshold >= 255) return hipSuccess;  // no byte pair is further apart
    const int aligned = (((uintptr_t)img | pitch) & 3) == 0;
    hipLaunchKernelGGL(sr_edge_seed_kernel, dim3((unsigned)(gx * gy)), dim3(kThreads), 0, stream, img, pitch, width,
                       height, gx, gy, threshold, grow, aligned, dev_mask);
    return hipGetLastError();
}

// The launch codes of the sample frame ((ss width) x (ss height), sgx x sgy
// workgroup tiles) for the flagged tiles of dev_mask: codes[0 .. sgx * sgy)
// with the flagged tiles' sample tiles at the front, in the order of the
// plain frame's n_order launch codes `order`, and -1 behind them. Copies the
// mask to user_mask when that is not null.
extern "C" hipError_t sr_adaptive_codes_device(const uint8_t* dev_mask, int width, int height, int ss, const int* order,
                                               int n_order, int* codes, uint8_t* user_mask, hipStream_t stream) {
    const int gx = (width + 15) / 16, gy = (height + 15) / 16;
    const long long sgx = ((long long)ss * width + 15) / 16, sgy = ((long long)ss * height + 15) / 16;
    if (width <= 0 || height <= 0 || ss < 1 || sgx * sgy > (1 << 22) || !order || n_order < gx * gy)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(codes, 0xff, (size_t)(sgx * sgy) * sizeof(int), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sr_adaptive_codes_kernel, dim3(1), dim3(kCodesThreads), 0, stream, dev_mask, gx * gy, gx, ss,
                       (int)sgx, (int)sgy, order, n_order, codes, user_mask);
    return hipGetLastError();
}

// The same selection in plain C++ on host memory.
extern "C" void sr_edge_tiles_host(const uint8_t* img, size_t pitch, int width, int height, int threshold, int grow,
                                   uint8_t* mask) {
    const int gx = (width + 15) / 16, gy = (height + 15) / 16;
    const size_t n = (size_t)gx * gy;
    for (size_t i = 0; i < n; i++) mask[i] = threshold < 0 ? 1 : 0;
    if (threshold < 0 || threshold >= 255) return;
    const auto at = [&](int x, int y) { return load_pixel(img + (size_t)y * pitch + (size_t)x * 4, false); };
    const auto seed = [&](int x, int y) { mask[(size_t)(y / 16) * gx + x / 16] = 1; };
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const uint32_t a = at(x, y);
            if (x + 1 < width && channel_distance(a, at(x + 1, y)) > threshold) seed(x, y), seed(x + 1, y);
            if (y + 1 < height && channel_distance(a, at(x, y + 1)) > threshold) seed(x, y), seed(x, y + 1);
        }
    for (int g = 0; g < grow; g++) {  // one 3x3 dilation per round; 2 marks this round's new tiles
        for (int ty = 0; ty < gy; ty++)
            for (int tx = 0; tx < gx; tx++) {
                if (mask[(size_t)ty * gx + tx]) continue;
                bool near = false;
                for (int dy = -1; dy <= 1 && !near; dy++)
                    for (int dx = -1; dx <= 1 && !near; dx++) {
                        const int nx = tx + dx, ny = ty + dy;
                        near = nx >= 0 && nx < gx && ny >= 0 && ny < gy && mask[(size_t)ny * gx + nx] == 1;
                    }
                if (near) mask[(size_t)ty * gx + tx] = 2;
            }
        for (size_t i = 0; i < n; i++) mask[i] = mask[i] ? 1 : 0;
    }
}
