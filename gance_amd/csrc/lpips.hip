// The kernels of the VGG16 LPIPS distance (gance_amd/stylegan2/lpips.py through torch.ops.gance.lpips_input, bias_relu,
// bias_relu_pool, lpips_layer and lpips_normalize). The thirteen convolutions are not here: they
// are gance_modconv3x3_forward / _backward with unit style and demodulation. fp32 NCHW, on the caller's stream, no host
// synchronisation, no atomics; every sum has one fixed order, so two runs give the same bits. The sum that ends in one number
// per sample (the distance of a tap) is accumulated in fp64 inside a block and in the finish kernel, as projection.hip does.
//
//   input      forward:  input_forward_kernel (area mean by R / S, (x - shift) / scale, zero channels 3 ... 15)
//              backward: input_backward_kernel (grad / (scale * factor^2) spread over the factor x factor cell)
//   bias/relu  forward:  bias_relu_kernel, bias_relu_pool_kernel (one thread per 2x2 window writes y and its maximum p)
//              backward: bias_relu_backward_kernel, bias_relu_pool_backward_kernel (the window's first largest y takes grad_p)
//   head       forward:  head_forward_kernel (per pixel n = |f|, sum_c lin_c (f_c / (n + 1e-10) - t_c)^2; per block one fp64
//                        partial), head_finish_kernel;  backward: head_backward_kernel (recomputes n and the dot product)
//   normalise            normalize_kernel (f / (n + 1e-10))
//
// The per-pixel kernels reduce over the channels as the noise-gradient kernel of synthesis_grad.hip does: a block is 64 positions
// x 4 channel groups (16 x 16 below 4096 positions), a thread sums its group's channels in rising order, and every thread of a
// position adds the groups' sums in rising order. `pixel_norm` is that sum for n, shared by the three kernels: the target
// features the normalise kernel wrote and the image features the head normalises agree to the bit where the inputs do.

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace gance_lpips {

constexpr int kThreads = 256;
constexpr int kMaxBatch = 65535;
constexpr int kInputChannels = 16;         // the input kernel's output: RGB + 13 zero channels (conv1_1 runs at Cin = 16)
constexpr int kWidePositions = 64;         // positions per block at 4096 positions and above
constexpr int kNarrowPositions = 16;       // ... and below
constexpr int kNarrowBelow = 4096;
constexpr float kNormEpsilon = 1e-10f;

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

// ---- the input ----

// out[b][c][y][x], c < 3: ((sum of the factor x factor cell, rows then columns) / factor^2 - shift_c) / scale_c; c >= 3: 0
__global__ __launch_bounds__(kThreads) void input_forward_kernel(const float* __restrict__ image, const float* __restrict__ shift,
                                                                 const float* __restrict__ scale, int resolution, int side, float* __restrict__ out) {
    const int at = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    const int plane = side * side;
    if (at >= kInputChannels * plane) return;
    const int c = at / plane, rest = at - c * plane;
    float value = 0.f;
    if (c < 3) {
        const int y = rest / side, x = rest - y * side, factor = resolution / side;
        const float* const cell = image + ((size_t)b * 3 + c) * resolution * resolution + (size_t)y * factor * resolution + x * factor;
        float sum = 0.f;
        for (int fy = 0; fy < factor; ++fy)
            for (int fx = 0; fx < factor; ++fx) sum += cell[(size_t)fy * resolution + fx];
        if (factor > 1) sum /= (float)(factor * factor);
        value = (sum - shift[c]) / scale[c];
    }
    out[(size_t)b * kInputChannels * plane + at] = value;
}

// grad_image[b][c][Y][X] = grad[b][c][Y / factor][X / factor] / (scale_c * factor^2)
__global__ __launch_bounds__(kThreads) void input_backward_kernel(const float* __restrict__ grad, const float* __restrict__ scale, int resolution,
                                                                  int side, float* __restrict__ grad_image) {
    const int at = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    const int plane = resolution * resolution;
    if (at >= 3 * plane) return;
    const int c = at / plane, rest = at - c * plane;
    const int Y = rest / resolution, X = rest - Y * resolution, factor = resolution / side;
    const float g = grad[((size_t)b * kInputChannels + c) * side * side + (size_t)(Y / factor) * side + X / factor];
    grad_image[(size_t)b * 3 * plane + at] = g / (scale[c] * (float)(factor * factor));
}

// ---- bias + ReLU (+ 2x2 max pool) ----

__global__ __launch_bounds__(kThreads) void bias_relu_kernel(const float* __restrict__ x, const float* __restrict__ bias, int channels, int plane,
                                                             float* __restrict__ y) {
    const int at = blockIdx.x * kThreads + threadIdx.x;
    if (at >= channels * plane) return;
    const size_t index = (size_t)blockIdx.y * channels * plane + at;
    y[index] = fmaxf(x[index] + bias[at / plane], 0.f);
}

__global__ __launch_bounds__(kThreads) void bias_relu_backward_kernel(const float* __restrict__ grad_y, const float* __restrict__ y, int per_sample,
                                                                      float* __restrict__ grad_x) {
    const int at = blockIdx.x * kThreads + threadIdx.x;
    if (at >= per_sample) return;
    const size_t index = (size_t)blockIdx.y * per_sample + at;
    grad_x[index] = y[index] > 0.f ? grad_y[index] : 0.f;
}

// the element of a 2x2 window (row-major a, c / d, f) that a max pool selects: the largest, the first of equals
__device__ __forceinline__ int selected(float a, float c, float d, float f) {
    int at = 0;
    float best = a;
    if (c > best) best = c, at = 1;
    if (d > best) best = d, at = 2;
    if (f > best) at = 3;
    return at;
}

// one thread per window: y = max(x + bias_c, 0) at its four positions, p = their maximum
__global__ __launch_bounds__(kThreads) void bias_relu_pool_kernel(const float* __restrict__ x, const float* __restrict__ bias, int channels, int side,
                                                                  float* __restrict__ y, float* __restrict__ p) {
    const int at = blockIdx.x * kThreads + threadIdx.x;
    const int half = side >> 1, windows = half * half;
    if (at >= channels * windows) return;
    const int c = at / windows, rest = at - c * windows, wy = rest / half, wx = rest - wy * half;
    const size_t plane = ((size_t)blockIdx.y * channels + c) * side * side;
    const size_t top = plane + (size_t)(2 * wy) * side + 2 * wx;
    const float shift = bias[c];
    const float a = fmaxf(x[top] + shift, 0.f), k = fmaxf(x[top + 1] + shift, 0.f);
    const float d = fmaxf(x[top + side] + shift, 0.f), f = fmaxf(x[top + side + 1] + shift, 0.f);
    y[top] = a, y[top + 1] = k, y[top + side] = d, y[top + side + 1] = f;
    p[(size_t)blockIdx.y * channels * windows + at] = fmaxf(fmaxf(a, k), fmaxf(d, f));
}

// grad_x = (y > 0) * (grad_y + grad_p at the window's selected element)
__global__ __launch_bounds__(kThreads) void bias_relu_pool_backward_kernel(const float* __restrict__ grad_y, const float* __restrict__ grad_p,
                                                                           const float* __restrict__ y, int channels, int side,
                                                                           float* __restrict__ grad_x) {
    const int at = blockIdx.x * kThreads + threadIdx.x;
    const int half = side >> 1, windows = half * half;
    if (at >= channels * windows) return;
    const int c = at / windows, rest = at - c * windows, wy = rest / half, wx = rest - wy * half;
    const size_t plane = ((size_t)blockIdx.y * channels + c) * side * side;
    const size_t top = plane + (size_t)(2 * wy) * side + 2 * wx;
    const size_t where[4] = {top, top + 1, top + side, top + side + 1};
    const float value[4] = {y[where[0]], y[where[1]], y[where[2]], y[where[3]]};
    const int chosen = selected(value[0], value[1], value[2], value[3]);
    const float pooled = grad_p[(size_t)blockIdx.y * channels * windows + at];
#pragma unroll
    for (int k = 0; k < 4; ++k) grad_x[where[k]] = value[k] > 0.f ? grad_y[where[k]] + (k == chosen ? pooled : 0.f) : 0.f;
}

// ---- the per-pixel kernels: PX positions x (kThreads / PX) channel groups per block ----

// sum over the channels of this thread's position of `mine` (the thread's own group's sum), groups in rising order; every
// thread of a position gets the same bits. `sums` is [kThreads] floats.
template <int PX>
__device__ __forceinline__ float over_groups(float mine, float* sums) {
    sums[threadIdx.x] = mine;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int g = 0; g < kThreads / PX; ++g) total += sums[g * PX + (threadIdx.x % PX)];
    __syncthreads();
    return total;
}

// n = sqrt(sum_c f_c^2) of this thread's position; `pixel` points at channel 0 of the position (or is unused when !valid)
template <int PX>
__device__ __forceinline__ float pixel_norm(const float* pixel, bool valid, int channels, size_t plane, float* sums) {
    float squares = 0.f;
    if (valid)
        for (int c = threadIdx.x / PX; c < channels; c += kThreads / PX) {
            const float value = pixel[(size_t)c * plane];
            squares = fmaf(value, value, squares);
        }
    return sqrtf(over_groups<PX>(squares, sums));
}

template <int PX>
__global__ __launch_bounds__(kThreads) void normalize_kernel(const float* __restrict__ f, int channels, int plane, float* __restrict__ out) {
    __shared__ float sums[kThreads];
    const int position = blockIdx.x * PX + threadIdx.x % PX;
    const bool valid = position < plane;
    const size_t first = (size_t)blockIdx.y * channels * plane + position;
    const float denominator = pixel_norm<PX>(f + first, valid, channels, plane, sums) + kNormEpsilon;
    if (!valid) return;
    for (int c = threadIdx.x / PX; c < channels; c += kThreads / PX) out[first + (size_t)c * plane] = f[first + (size_t)c * plane] / denominator;
}

// partial[b][block] = sum over the block's positions and the channels of lin_c (f_c / (n + 1e-10) - t_c)^2
template <int PX>
__global__ __launch_bounds__(kThreads) void head_forward_kernel(const float* __restrict__ f, const float* __restrict__ target,
                                                                const float* __restrict__ lin, int channels, int plane, double* __restrict__ partial) {
    __shared__ float sums[kThreads];
    __shared__ double block_sums[kThreads];
    const int position = blockIdx.x * PX + threadIdx.x % PX;
    const bool valid = position < plane;
    const size_t first = (size_t)blockIdx.y * channels * plane + position;
    const float denominator = pixel_norm<PX>(f + first, valid, channels, plane, sums) + kNormEpsilon;
    double weighted = 0.;
    if (valid)
        for (int c = threadIdx.x / PX; c < channels; c += kThreads / PX) {
            const float difference = f[first + (size_t)c * plane] / denominator - target[first + (size_t)c * plane];
            weighted += (double)lin[c] * ((double)difference * (double)difference);
        }
    weighted = block_sum(weighted, block_sums);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = weighted;
}

// dist[b] = (the partials of sample b: per-thread strided sums, then a tree) / positions
__global__ __launch_bounds__(kThreads) void head_finish_kernel(const double* __restrict__ partial, int blocks, int plane, float* __restrict__ dist) {
    __shared__ double block_sums[kThreads];
    double sum = 0.;
    for (int k = threadIdx.x; k < blocks; k += kThreads) sum += partial[(size_t)blockIdx.x * blocks + k];
    sum = block_sum(sum, block_sums);
    if (threadIdx.x == 0) dist[blockIdx.x] = (float)(sum / (double)plane);
}

// With u = f / (n + eps), a_c = 2 lin_c (u_c - t_c) and dot = sum_c a_c f_c:
//   grad_f_k = grad_d / positions * (a_k / (n + eps) - dot * f_k / (n (n + eps)^2)),   the second term 0 where n = 0
// (d n / d f is taken as 0 at f = 0, its limit along every axis being bounded and f_k itself 0 there).
template <int PX>
__global__ __launch_bounds__(kThreads) void head_backward_kernel(const float* __restrict__ grad_dist, const float* __restrict__ f,
                                                                 const float* __restrict__ target, const float* __restrict__ lin, int channels,
                                                                 int plane, float* __restrict__ grad_f) {
    __shared__ float sums[kThreads];
    const int position = blockIdx.x * PX + threadIdx.x % PX;
    const bool valid = position < plane;
    const size_t first = (size_t)blockIdx.y * channels * plane + position;
    const float n = pixel_norm<PX>(f + first, valid, channels, plane, sums);
    const float denominator = n + kNormEpsilon;
    float mine = 0.f;
    if (valid)
        for (int c = threadIdx.x / PX; c < channels; c += kThreads / PX) {
            const float value = f[first + (size_t)c * plane];
            mine += 2.f * lin[c] * (value / denominator - target[first + (size_t)c * plane]) * value;
        }
    const float dot = over_groups<PX>(mine, sums);
    if (!valid) return;
    const float g = grad_dist[blockIdx.y] / (float)plane;
    const float along = n > 0.f ? dot / (n * denominator * denominator) : 0.f;
    for (int c = threadIdx.x / PX; c < channels; c += kThreads / PX) {
        const float value = f[first + (size_t)c * plane];
        const float a = 2.f * lin[c] * (value / denominator - target[first + (size_t)c * plane]);
        grad_f[first + (size_t)c * plane] = g * (a / denominator - along * value);
    }
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

static int check_channels(const char* function, int32_t channels) {
    if (channels < 16 || channels > 512 || channels % 16 != 0)
        return invalid(function, "channels must be a multiple of 16 in [16, 512], got " + std::to_string(channels));
    return GANCE_OK;
}

static int check_side(const char* function, const char* what, int32_t side) {
    if (side < 4 || side > 1024) return invalid(function, std::string(what) + " must be in [4, 1024], got " + std::to_string(side));
    return GANCE_OK;
}

static int check_input_sides(const char* function, int32_t resolution, int32_t side) {
    if (const int status = check_side(function, "resolution", resolution)) return status;
    if (const int status = check_side(function, "side", side)) return status;
    if (resolution % side != 0)
        return invalid(function, "resolution must be a multiple of side, got " + std::to_string(resolution) + " and " + std::to_string(side));
    return GANCE_OK;
}

static int check_pool(const char* function, int32_t side, int32_t pool) {
    if (pool != 0 && side % 2 != 0) return invalid(function, "side must be even with pool, got " + std::to_string(side));
    return GANCE_OK;
}

static int positions_per_block(int plane) { return plane < kNarrowBelow ? kNarrowPositions : kWidePositions; }
static unsigned head_blocks(int32_t side) {
    const int plane = side * side, px = positions_per_block(plane);
    return (unsigned)((plane + px - 1) / px);
}
static uint64_t head_workspace(int32_t batch, int32_t side) { return (uint64_t)batch * head_blocks(side) * sizeof(double); }

static unsigned blocks_of(int64_t elements) { return (unsigned)((elements + kThreads - 1) / kThreads); }

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

}  // namespace gance_lpips

extern "C" {

int gance_lpips_input_forward(const float* d_image, const float* d_shift, const float* d_scale, int32_t batch, int32_t resolution, int32_t side,
                              float* d_out, void* stream_ptr) {
    using namespace gance_lpips;
    static const char* const kName = "gance_lpips_input_forward";
    if (const int status = check_pointers(kName, {d_image, d_shift, d_scale, d_out})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_input_sides(kName, resolution, side)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_image));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    input_forward_kernel<<<dim3(blocks_of((int64_t)kInputChannels * side * side), batch), kThreads, 0, (hipStream_t)stream_ptr>>>(
        d_image, d_shift, d_scale, resolution, side, d_out);
    return launched(kName);
}

int gance_lpips_input_backward(const float* d_grad, const float* d_scale, int32_t batch, int32_t resolution, int32_t side, float* d_grad_image,
                               void* stream_ptr) {
    using namespace gance_lpips;
    static const char* const kName = "gance_lpips_input_backward";
    if (const int status = check_pointers(kName, {d_grad, d_scale, d_grad_image})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_input_sides(kName, resolution, side)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_grad));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    input_backward_kernel<<<dim3(blocks_of((int64_t)3 * resolution * resolution), batch), kThreads, 0, (hipStream_t)stream_ptr>>>(
        d_grad, d_scale, resolution, side, d_grad_image);
    return launched(kName);
}

int gance_bias_relu_forward(const float* d_x, const float* d_bias, int32_t batch, int32_t channels, int32_t side, int32_t pool, float* d_y,
                            float* d_p, void* stream_ptr) {
    using namespace gance_lpips;
    static const char* const kName = "gance_bias_relu_forward";
    if (const int status = check_pointers(kName, {d_x, d_bias, d_y})) return status;
    if (pool != 0)
        if (const int status = check_pointers(kName, {d_p})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_channels(kName, channels)) return status;
    if (const int status = check_side(kName, "side", side)) return status;
    if (const int status = check_pool(kName, side, pool)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_x));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (pool != 0)
        bias_relu_pool_kernel<<<dim3(blocks_of((int64_t)channels * (side / 2) * (side / 2)), batch), kThreads, 0, stream>>>(d_x, d_bias, channels,
                                                                                                                             side, d_y, d_p);
    else
        bias_relu_kernel<<<dim3(blocks_of((int64_t)channels * side * side), batch), kThreads, 0, stream>>>(d_x, d_bias, channels, side * side, d_y);
    return launched(kName);
}

int gance_bias_relu_backward(const float* d_grad_y, const float* d_grad_p, const float* d_y, int32_t batch, int32_t channels, int32_t side,
                             int32_t pool, float* d_grad_x, void* stream_ptr) {
    using namespace gance_lpips;
    static const char* const kName = "gance_bias_relu_backward";
    if (const int status = check_pointers(kName, {d_grad_y, d_y, d_grad_x})) return status;
    if (pool != 0)
        if (const int status = check_pointers(kName, {d_grad_p})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_channels(kName, channels)) return status;
    if (const int status = check_side(kName, "side", side)) return status;
    if (const int status = check_pool(kName, side, pool)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_y));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (pool != 0)
        bias_relu_pool_backward_kernel<<<dim3(blocks_of((int64_t)channels * (side / 2) * (side / 2)), batch), kThreads, 0, stream>>>(
            d_grad_y, d_grad_p, d_y, channels, side, d_grad_x);
    else
        bias_relu_backward_kernel<<<dim3(blocks_of((int64_t)channels * side * side), batch), kThreads, 0, stream>>>(d_grad_y, d_y,
                                                                                                                    channels * side * side, d_grad_x);
    return launched(kName);
}

int gance_lpips_layer_workspace_bytes(int32_t batch, int32_t side, uint64_t* workspace_bytes) {
    using namespace gance_lpips;
    static const char* const kName = "gance_lpips_layer_workspace_bytes";
    if (workspace_bytes == nullptr) return invalid(kName, "NULL pointer");
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_side(kName, "side", side)) return status;
    *workspace_bytes = head_workspace(batch, side);
    return GANCE_OK;
}

int gance_lpips_layer_forward(const float* d_f, const float* d_target, const float* d_lin, int32_t batch, int32_t channels, int32_t side,
                              float* d_dist, void* d_workspace, uint64_t workspace_bytes, void* stream_ptr) {
    using namespace gance_lpips;
    static const char* const kName = "gance_lpips_layer_forward";
    if (const int status = check_pointers(kName, {d_f, d_target, d_lin, d_dist, d_workspace})) return status;
    if ((uintptr_t)d_workspace % alignof(double) != 0) return invalid(kName, "misaligned workspace (8-byte alignment needed)");
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_channels(kName, channels)) return status;
    if (const int status = check_side(kName, "side", side)) return status;
    const uint64_t needed = head_workspace(batch, side);
    if (workspace_bytes < needed)
        return invalid(kName, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed) +
                                  " needed (gance_lpips_layer_workspace_bytes)");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_f));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int plane = side * side;
    const unsigned blocks = head_blocks(side);
    double* const partial = (double*)d_workspace;
    if (positions_per_block(plane) == kNarrowPositions)
        head_forward_kernel<kNarrowPositions><<<dim3(blocks, batch), kThreads, 0, stream>>>(d_f, d_target, d_lin, channels, plane, partial);
    else
        head_forward_kernel<kWidePositions><<<dim3(blocks, batch), kThreads, 0, stream>>>(d_f, d_target, d_lin, channels, plane, partial);
    head_finish_kernel<<<batch, kThreads, 0, stream>>>(partial, (int)blocks, plane, d_dist);
    return launched(kName);
}

int gance_lpips_layer_backward(const float* d_grad_dist, const float* d_f, const float* d_target, const float* d_lin, int32_t batch,
                               int32_t channels, int32_t side, float* d_grad_f, void* stream_ptr) {
    using namespace gance_lpips;
    static const char* const kName = "gance_lpips_layer_backward";
    if (const int status = check_pointers(kName, {d_grad_dist, d_f, d_target, d_lin, d_grad_f})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_channels(kName, channels)) return status;
    if (const int status = check_side(kName, "side", side)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_f));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int plane = side * side;
    if (positions_per_block(plane) == kNarrowPositions)
        head_backward_kernel<kNarrowPositions><<<dim3(head_blocks(side), batch), kThreads, 0, stream>>>(d_grad_dist, d_f, d_target, d_lin, channels,
                                                                                                        plane, d_grad_f);
    else
        head_backward_kernel<kWidePositions><<<dim3(head_blocks(side), batch), kThreads, 0, stream>>>(d_grad_dist, d_f, d_target, d_lin, channels,
                                                                                                      plane, d_grad_f);
    return launched(kName);
}

int gance_lpips_normalize(const float* d_f, int32_t batch, int32_t channels, int32_t side, float* d_out, void* stream_ptr) {
    using namespace gance_lpips;
    static const char* const kName = "gance_lpips_normalize";
    if (const int status = check_pointers(kName, {d_f, d_out})) return status;
    if (const int status = check_batch(kName, batch)) return status;
    if (const int status = check_channels(kName, channels)) return status;
    if (const int status = check_side(kName, "side", side)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_f));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int plane = side * side;
    if (positions_per_block(plane) == kNarrowPositions)
        normalize_kernel<kNarrowPositions><<<dim3(head_blocks(side), batch), kThreads, 0, stream>>>(d_f, channels, plane, d_out);
    else
        normalize_kernel<kWidePositions><<<dim3(head_blocks(side), batch), kThreads, 0, stream>>>(d_f, channels, plane, d_out);
    return launched(kName);
}

}  // extern "C"
