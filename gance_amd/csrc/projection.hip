// Projection's loss kernels (gance_amd/stylegan2/projector.py through torch.ops.gance.noise_regularizer and
// torch.ops.gance.pyramid_distance): the multi-scale autocorrelation penalty of StyleGAN2's
// projector over one noise plane per sample, and a weight-free multi-scale squared image distance. fp32, on the caller's
// stream, no host synchronisation, no atomics: every sum is per-thread strided partials, a tree over the block, and a
// fixed-order sum of the blocks' partials, so two runs give the same bits. The data is fp32; the sums that end in one number
// per sample (the correlations, the distance) are accumulated in fp64 inside a block and in the finish kernels, and rounded
// to fp32 once per block and once at the end: a scalar has no neighbours to average its rounding with, and a handful of
// fp64 additions per thread cost nothing beside the reads.
//
// Both are pyramids of 2x2 means whose coarsest level is 8 x 8 (or the input itself when its side is 4 or 8), so a tile of
// side / 8 level-0 pixels ends in exactly one coarsest pixel: one block owns a tile through every level.
//
//   regulariser  forward:  pyramid_kernel (levels 1 ... of every plane into the workspace), correlation_kernel (per level and
//                          segment: sum v * roll(v, 1) along W and along H), regularizer_finish_kernel (means, reg)
//                backward: regularizer_backward_kernel (one thread per 2x2 quad of level 0 walks up its ancestors)
//   distance     forward:  distance_tile_kernel (area mean, difference, pyramid, weighted squares per tile),
//                          distance_finish_kernel;  backward: distance_backward_kernel (one thread per image pixel)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace gance_proj {

constexpr int kThreads = 256;
constexpr int kMaxBatch = 65535;
constexpr int kMaxLevels = 8;            // 1024 -> 8
constexpr int kCorrSegments = 256;       // most partial sums per level of a plane
constexpr int kCorrSegmentPositions = 4096;
constexpr int kTiles = 64;               // 8 x 8 tiles per plane

__device__ __forceinline__ double block_sum(double value, double* sums) {
    sums[threadIdx.x] = value;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) sums[threadIdx.x] += sums[threadIdx.x + half];
        __syncthreads();
    }
    const double total = sums[0];
    __syncthreads();
    return total;
}

__host__ __device__ inline int levels_of(int side) {  // sides side, side / 2, ... 8; one level for 4 and 8
    int levels = 1;
    while (side > 8) side >>= 1, ++levels;
    return levels;
}

// floats of the levels first ... last - 1 of one plane (level l has (side >> l)^2)
__host__ __device__ inline size_t level_offset(int side, int first, int last) {
    size_t total = 0;
    for (int l = first; l < last; ++l) total += (size_t)(side >> l) * (side >> l);
    return total;
}

// ---- the noise regulariser ----

// levels 1 ... L - 1 of every plane: block (tile, b) owns a side / 8 tile of level 0. pyramid [B][levels 1 ...] floats.
__global__ __launch_bounds__(kThreads) void pyramid_kernel(const float* __restrict__ v, int side, int levels, float* __restrict__ pyramid) {
    __shared__ float even[64 * 64], odd[32 * 32];
    const int tile = side >> 3, b = blockIdx.y;
    const int ty = (blockIdx.x >> 3) * tile, tx = (blockIdx.x & 7) * tile;
    const float* const plane = v + (size_t)b * side * side;
    float* const levels_out = pyramid + (size_t)b * level_offset(side, 1, levels);
    for (int l = 1; l < levels; ++l) {
        const int t = tile >> l, s = side >> l;  // this level's tile and plane sides
        float* const dst = (l & 1) ? even : odd;
        const float* const src = (l & 1) ? odd : even;
        float* const out = levels_out + level_offset(side, 1, l);
        for (int e = threadIdx.x; e < t * t; e += kThreads) {
            const int y = e / t, x = e - y * t;
            float a, c, d, f;
            if (l == 1) {
                const float* const q = plane + (size_t)(ty + 2 * y) * side + tx + 2 * x;
                a = q[0], c = q[1], d = q[side], f = q[side + 1];
            } else {
                const float* const q = src + (2 * y) * (2 * t) + 2 * x;
                a = q[0], c = q[1], d = q[2 * t], f = q[2 * t + 1];
            }
            const float mean = ((a + c) + (d + f)) * 0.25f;
            dst[y * t + x] = mean;
            out[(size_t)((ty >> l) + y) * s + (tx >> l) + x] = mean;
        }
        __syncthreads();
    }
}

// partial[b][l][dir][seg] = sum over the segment's positions of v_l * roll(v_l, 1) along W (dir 0) and H (dir 1); the roll wraps
__global__ __launch_bounds__(kThreads) void correlation_kernel(const float* __restrict__ v, const float* __restrict__ pyramid, int side, int levels,
                                                               float* __restrict__ partial) {
    __shared__ double sums[kThreads];
    const int seg = blockIdx.x, l = blockIdx.y, b = blockIdx.z;
    const int s = side >> l, positions = s * s;
    const int segments = min(kCorrSegments, (positions + kCorrSegmentPositions - 1) / kCorrSegmentPositions);
    if (seg >= segments) return;
    const int segment = (positions + segments - 1) / segments;
    const float* const plane =
        l == 0 ? v + (size_t)b * side * side : pyramid + (size_t)b * level_offset(side, 1, levels) + level_offset(side, 1, l);
    const int first = seg * segment, last = min(first + segment, positions);
    double along_w = 0., along_h = 0.;
    for (int at = first + threadIdx.x; at < last; at += kThreads) {
        const int y = at / s, x = at - y * s;
        const double value = plane[at];
        along_w += value * plane[y * s + ((x + s - 1) & (s - 1))];
        along_h += value * plane[((y + s - 1) & (s - 1)) * s + x];
    }
    along_w = block_sum(along_w, sums);
    along_h = block_sum(along_h, sums);
    if (threadIdx.x == 0) {
        float* const out = partial + ((size_t)b * levels + l) * 2 * kCorrSegments;
        out[seg] = (float)along_w;
        out[kCorrSegments + seg] = (float)along_h;
    }
}

// means[b][l][dir] = (the partials in rising order) / positions; reg[b] = sum over l, dir (in that order) of mean^2
__global__ void regularizer_finish_kernel(const float* __restrict__ partial, int side, int levels, float* __restrict__ means, float* __restrict__ reg) {
    __shared__ double mean[2 * kMaxLevels];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 2 * levels) {
        const int l = t >> 1, s = side >> l, positions = s * s;
        const int segments = min(kCorrSegments, (positions + kCorrSegmentPositions - 1) / kCorrSegmentPositions);
        const float* const in = partial + ((size_t)b * levels * 2 + t) * kCorrSegments;
        double sum = 0.;
        for (int seg = 0; seg < segments; ++seg) sum += in[seg];
        mean[t] = sum / (double)positions;
        means[(size_t)b * levels * 2 + t] = (float)mean[t];
    }
    __syncthreads();
    if (t == 0) {
        double sum = 0.;
        for (int k = 0; k < 2 * levels; ++k) sum += mean[k] * mean[k];
        reg[b] = (float)sum;
    }
}

// d reg / d v: level l gives its pixels grad_reg * 2 mean_dir / n_l * (both neighbours along dir), and a 2x2 mean hands a quarter
// to each input, so a level-0 pixel receives 0.25^l of its ancestor's value at level l. One thread per 2x2 quad of level 0
// (a quad shares every ancestor), coarsest level first.
__global__ __launch_bounds__(kThreads) void regularizer_backward_kernel(const float* __restrict__ grad_reg, const float* __restrict__ v,
                                                                        const float* __restrict__ pyramid, const float* __restrict__ means, int side,
                                                                        int levels, float* __restrict__ grad_v) {
    const int half = side >> 1, b = blockIdx.y;
    const int quad = blockIdx.x * kThreads + threadIdx.x;
    if (quad >= half * half) return;
    const int qy = quad / half, qx = quad - qy * half;
    const float g = grad_reg[b];
    const float* const pyramid_b = pyramid + (size_t)b * level_offset(side, 1, levels);
    float coarse = 0.f;
    for (int l = levels - 1; l >= 1; --l) {
        const int s = side >> l, y = qy >> (l - 1), x = qx >> (l - 1);
        const float* const plane = pyramid_b + level_offset(side, 1, l);
        const float scale = g * 2.f / ((float)s * (float)s) * (1.f / (float)(1 << (2 * l)));
        const float cw = scale * means[((size_t)b * levels + l) * 2], ch = scale * means[((size_t)b * levels + l) * 2 + 1];
        coarse += cw * (plane[y * s + ((x + s - 1) & (s - 1))] + plane[y * s + ((x + 1) & (s - 1))]) +
                  ch * (plane[((y + s - 1) & (s - 1)) * s + x] + plane[((y + 1) & (s - 1)) * s + x]);
    }
    const float* const plane = v + (size_t)b * side * side;
    const float scale = g * 2.f / ((float)side * (float)side);
    const float cw = scale * means[(size_t)b * levels * 2], ch = scale * means[(size_t)b * levels * 2 + 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * qy + (k >> 1), x = 2 * qx + (k & 1), m = side - 1;
        grad_v[((size_t)b * side + y) * side + x] = coarse + (cw * (plane[(size_t)y * side + ((x + m) & m)] + plane[(size_t)y * side + ((x + 1) & m)]) +
                                                              ch * (plane[(size_t)((y + m) & m) * side + x] + plane[(size_t)((y + 1) & m) * side + x]));
    }
}

// ---- the pyramid distance ----

// block (tile, c, b): d_0 = (area mean of (image + 1) * 127.5 - target) / 255 over the tile, then its 2x2 means down to one pixel;
// every level goes to `saved` [B][3][levels 0 ...] for the backward, and partial[b][c][tile] = sum_l sum_tile d_l^2 / (3 n_l)
__global__ __launch_bounds__(kThreads) void distance_tile_kernel(const float* __restrict__ image, const float* __restrict__ target, int resolution,
                                                                 int side, int levels, float* __restrict__ saved, float* __restrict__ partial) {
    __shared__ float even[32 * 32], odd[16 * 16];
    __shared__ double sums[kThreads];
    const int factor = resolution / side;
    const int tile = max(side >> 3, 1), tiles_across = side / tile;  // side 8: 8 x 8 tiles of one pixel
    const int c = blockIdx.y, b = blockIdx.z;
    const int ty = (blockIdx.x / tiles_across) * tile, tx = (blockIdx.x % tiles_across) * tile;
    const float* const image_plane = image + ((size_t)b * 3 + c) * resolution * resolution;
    const float* const target_plane = target + ((size_t)b * 3 + c) * side * side;
    float* const saved_plane = saved + ((size_t)b * 3 + c) * level_offset(side, 0, levels);
    const float area = 1.f / (float)(factor * factor);
    double weighted = 0.;
    for (int l = 0; l < levels; ++l) {
        const int t = tile >> l, s = side >> l;
        float* const dst = (l & 1) ? odd : even;
        const float* const src = (l & 1) ? even : odd;
        float* const out = saved_plane + level_offset(side, 0, l);
        const double weight = 1. / (3. * (double)s * (double)s);
        for (int e = threadIdx.x; e < t * t; e += kThreads) {
            const int y = e / t, x = e - y * t;
            float value;
            if (l == 0) {
                float sum = 0.f;
                for (int fy = 0; fy < factor; ++fy) {
                    const float* const row = image_plane + (size_t)((ty + y) * factor + fy) * resolution + (tx + x) * factor;
                    for (int fx = 0; fx < factor; ++fx) sum += (row[fx] + 1.f) * 127.5f;
                }
                value = (sum * area - target_plane[(size_t)(ty + y) * side + tx + x]) / 255.f;  // (a true division: 1 / 255 rounded would bias every d alike)
            } else {
                const float* const q = src + (2 * y) * (2 * t) + 2 * x;
                value = ((q[0] + q[1]) + (q[2 * t] + q[2 * t + 1])) * 0.25f;
            }
            dst[y * t + x] = value;
            out[(size_t)((ty >> l) + y) * s + (tx >> l) + x] = value;
            weighted += (double)value * (double)value * weight;
        }
        __syncthreads();
    }
    weighted = block_sum(weighted, sums);
    if (threadIdx.x == 0) partial[((size_t)b * 3 + c) * kTiles + blockIdx.x] = (float)weighted;
}

// dist[b] = the 3 x 64 tile partials of sample b in rising order
__global__ __launch_bounds__(kThreads) void distance_finish_kernel(const float* __restrict__ partial, int batch, float* __restrict__ dist) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= batch) return;
    double sum = 0.;
    for (int k = 0; k < 3 * kTiles; ++k) sum += partial[(size_t)b * 3 * kTiles + k];
    dist[b] = (float)sum;
}

// grad_image[b][c][Y][X] = grad_dist[b] * 127.5 / 255 / factor^2 * sum_l 2 d_l[ancestor] / (3 n_l) * 0.25^l, coarsest level first
__global__ __launch_bounds__(kThreads) void distance_backward_kernel(const float* __restrict__ grad_dist, const float* __restrict__ saved,
                                                                     int resolution, int side, int levels, size_t total, float* __restrict__ grad_image) {
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    const int factor = resolution / side;
    const int X = (int)(at % resolution), Y = (int)((at / resolution) % resolution);
    const size_t plane = at / ((size_t)resolution * resolution);  // b * 3 + c
    const int y = Y / factor, x = X / factor;
    const float* const saved_plane = saved + plane * level_offset(side, 0, levels);
    float sum = 0.f;
    for (int l = levels - 1; l >= 0; --l) {
        const int s = side >> l;
        sum += saved_plane[level_offset(side, 0, l) + (size_t)(y >> l) * s + (x >> l)] * (2.f / (3.f * (float)s * (float)s) / (float)(1 << (2 * l)));
    }
    grad_image[at] = grad_dist[plane / 3] * (0.5f / (float)(factor * factor)) * sum;
}

// ---- host side ----

static int invalid(const char* function, const std::string& message) {
    return gance::set_last_error(GANCE_ERR_INVALID_ARGUMENT, std::string(function) + ": " + message);
}

static int check_pointers(const char* function, std::initializer_list<const void*> required) {
    for (const void* pointer : required)
        if (pointer == nullptr) return invalid(function, "NULL pointer");
    for (const void* pointer : required)
        if ((uintptr_t)pointer % alignof(float) != 0) return invalid(function, "misaligned pointer (float32 data must be 4-byte aligned)");
    return GANCE_OK;
}

static int check_batch(const char* function, int32_t batch) {
    if (batch < 1 || batch > kMaxBatch) return invalid(function, "batch must be in [1, " + std::to_string(kMaxBatch) + "], got " + std::to_string(batch));
    return GANCE_OK;
}

static int check_side(const char* function, const char* what, int32_t side, int32_t least, int32_t most) {
    if (side < least || side > most || (side & (side - 1)) != 0)
        return invalid(function, std::string(what) + " must be a power of two in [" + std::to_string(least) + ", " + std::to_string(most) + "], got " +
                                     std::to_string(side));
    return GANCE_OK;
}

static uint64_t round16(uint64_t bytes) { return (bytes + 15) / 16 * 16; }

// regulariser workspace: [the correlation partials [B][L][2][kCorrSegments]][the pyramid's levels 1 ... of every plane]
static uint64_t regularizer_partial_bytes(int32_t batch, int32_t side) {
    return round16((uint64_t)batch * levels_of(side) * 2 * kCorrSegments * sizeof(float));
}
static uint64_t regularizer_workspace(int32_t batch, int32_t side) {
    return regularizer_partial_bytes(batch, side) + round16((uint64_t)batch * level_offset(side, 1, levels_of(side)) * sizeof(float));
}

// distance workspace: [the tile partials [B][3][kTiles]][the pyramid of differences, levels 0 ..., [B][3]]
static int distance_side(int32_t resolution) { return std::min(resolution, 256); }
static uint64_t distance_partial_bytes(int32_t batch) { return round16((uint64_t)batch * 3 * kTiles * sizeof(float)); }
static uint64_t distance_workspace(int32_t batch, int32_t resolution) {
    const int side = distance_side(resolution);
    return distance_partial_bytes(batch) + round16((uint64_t)batch * 3 * level_offset(side, 0, levels_of(side)) * sizeof(float));
}

static int no_device() {
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return gance::set_last_error(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    return GANCE_OK;
}

static int hip_failure(const char* function, const char* what, hipError_t status) {
    return gance::set_last_error(GANCE_ERR_HIP, std::string(function) + ": " + what + ": " + hipGetErrorString(status));
}

static int launched(const char* function) {
    const hipError_t status = hipGetLastError();
    return status == hipSuccess ? GANCE_OK : hip_failure(function, "launch", status);
}

static int short_workspace(const char* function, uint64_t given, uint64_t needed, const char* sizer) {
    return invalid(function, "workspace of " + std::to_string(given) + " bytes, " + std::to_string(needed) + " needed (" + sizer + ")");
}

}  // namespace gance_proj

extern "C" {

int gance_noise_regularizer_workspace_bytes(int32_t batch, int32_t side, uint64_t* workspace_bytes) {
    using namespace gance_proj;
    static const char* const kName = "gance_noise_regularizer_workspace_bytes";
    if (workspace_bytes == nullptr) return invalid(kName, "NULL pointer");
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_side(kName, "side", side, 4, 1024)) return status;
    *workspace_bytes = regularizer_workspace(batch, side);
    return GANCE_OK;
}

int gance_noise_regularizer_forward(const float* d_noise, int32_t batch, int32_t side, float* d_reg, float* d_means, void* d_workspace,
                                    uint64_t workspace_bytes, void* stream_ptr) {
    using namespace gance_proj;
    static const char* const kName = "gance_noise_regularizer_forward";
    if (const int status = check_pointers(kName, {d_noise, d_reg, d_means, d_workspace})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_side(kName, "side", side, 4, 1024)) return status;
    const uint64_t needed = regularizer_workspace(batch, side);
    if (workspace_bytes < needed) return short_workspace(kName, workspace_bytes, needed, "gance_noise_regularizer_workspace_bytes");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_noise));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int levels = levels_of(side);
    float* const partial = (float*)d_workspace;
    float* const pyramid = (float*)((char*)d_workspace + regularizer_partial_bytes(batch, side));
    if (levels > 1) pyramid_kernel<<<dim3(kTiles, batch), kThreads, 0, stream>>>(d_noise, side, levels, pyramid);
    const int positions = side * side;
    const int segments = std::min(kCorrSegments, (positions + kCorrSegmentPositions - 1) / kCorrSegmentPositions);
    correlation_kernel<<<dim3(segments, levels, batch), kThreads, 0, stream>>>(d_noise, pyramid, side, levels, partial);
    regularizer_finish_kernel<<<batch, 64, 0, stream>>>(partial, side, levels, d_means, d_reg);
    return launched(kName);
}

int gance_noise_regularizer_backward(const float* d_grad_reg, const float* d_noise, const float* d_means, const void* d_workspace,
                                     uint64_t workspace_bytes, int32_t batch, int32_t side, float* d_grad_noise, void* stream_ptr) {
    using namespace gance_proj;
    static const char* const kName = "gance_noise_regularizer_backward";
    if (const int status = check_pointers(kName, {d_grad_reg, d_noise, d_means, d_workspace, d_grad_noise})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_side(kName, "side", side, 4, 1024)) return status;
    const uint64_t needed = regularizer_workspace(batch, side);
    if (workspace_bytes < needed) return short_workspace(kName, workspace_bytes, needed, "gance_noise_regularizer_workspace_bytes");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_noise));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    const float* const pyramid = (const float*)((const char*)d_workspace + regularizer_partial_bytes(batch, side));
    const unsigned quads = (unsigned)((side / 2) * (side / 2));
    regularizer_backward_kernel<<<dim3((quads + kThreads - 1) / kThreads, batch), kThreads, 0, (hipStream_t)stream_ptr>>>(
        d_grad_reg, d_noise, pyramid, d_means, side, levels_of(side), d_grad_noise);
    return launched(kName);
}

int gance_pyramid_distance_workspace_bytes(int32_t batch, int32_t resolution, uint64_t* workspace_bytes) {
    using namespace gance_proj;
    static const char* const kName = "gance_pyramid_distance_workspace_bytes";
    if (workspace_bytes == nullptr) return invalid(kName, "NULL pointer");
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_side(kName, "resolution", resolution, 8, 1024)) return status;
    *workspace_bytes = distance_workspace(batch, resolution);
    return GANCE_OK;
}

int gance_pyramid_distance_forward(const float* d_image, const float* d_target, int32_t batch, int32_t resolution, float* d_dist, void* d_workspace,
                                   uint64_t workspace_bytes, void* stream_ptr) {
    using namespace gance_proj;
    static const char* const kName = "gance_pyramid_distance_forward";
    if (const int status = check_pointers(kName, {d_image, d_target, d_dist, d_workspace})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_side(kName, "resolution", resolution, 8, 1024)) return status;
    const uint64_t needed = distance_workspace(batch, resolution);
    if (workspace_bytes < needed) return short_workspace(kName, workspace_bytes, needed, "gance_pyramid_distance_workspace_bytes");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_image));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int side = distance_side(resolution);
    float* const partial = (float*)d_workspace;
    float* const saved = (float*)((char*)d_workspace + distance_partial_bytes(batch));
    distance_tile_kernel<<<dim3(kTiles, 3, batch), kThreads, 0, stream>>>(d_image, d_target, resolution, side, levels_of(side), saved, partial);
    distance_finish_kernel<<<(batch + kThreads - 1) / kThreads, kThreads, 0, stream>>>(partial, batch, d_dist);
    return launched(kName);
}

int gance_pyramid_distance_backward(const float* d_grad_dist, const void* d_workspace, uint64_t workspace_bytes, int32_t batch, int32_t resolution,
                                    float* d_grad_image, void* stream_ptr) {
    using namespace gance_proj;
    static const char* const kName = "gance_pyramid_distance_backward";
    if (const int status = check_pointers(kName, {d_grad_dist, d_workspace, d_grad_image})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_side(kName, "resolution", resolution, 8, 1024)) return status;
    if ((int64_t)batch * 3 * resolution * resolution > (int64_t)0x7FFFFFFF * kThreads)
        return invalid(kName, "batch of " + std::to_string(batch) + " is more than one call's grid at this size");
    const uint64_t needed = distance_workspace(batch, resolution);
    if (workspace_bytes < needed) return short_workspace(kName, workspace_bytes, needed, "gance_pyramid_distance_workspace_bytes");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_grad_image));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    const int side = distance_side(resolution);
    const float* const saved = (const float*)((const char*)d_workspace + distance_partial_bytes(batch));
    const size_t total = (size_t)batch * 3 * resolution * resolution;
    distance_backward_kernel<<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0, (hipStream_t)stream_ptr>>>(
        d_grad_dist, saved, resolution, side, levels_of(side), total, d_grad_image);
    return launched(kName);
}

}  // extern "C"
