// The 3-D view of the synthesis inputs in HBM: gance_debug_scatter3d_u8 and gance_debug_draw_scatter3d_u8 of
// include/gance_hip.h.
//
// The cloud of every input vector of a run (one point per element: x = sample number i, y = vector number n, z = value)
// is the same on every frame; only a red marker moves along y. So the cloud is rasterised ONCE per run into a template
// [side][side][3] with a depth test, and a frame is a copy of the template (16 bytes per lane) with one stamp.
//
// The rasterisation rule, everything in double, in the order written, no contraction (this
// file is compiled with -ffp-contract=off):
//   unit cube        u_k = (p_k - lo_k) / (hi_k - lo_k) - 0.5 for k = x, y, z
//   projection       sx = (right[0] u_x + right[1] u_y) + right[2] u_z; sy with `up`, depth with `toward`: orthographic,
//                    the view vectors come from the host (the kernels call neither sin nor cos)
//   half extent      H(w) = ((|w[0]| + |w[1]|) + |w[2]|) / 2: what a projected coordinate reaches over the unit cube
//   value -> pixel   column = axis.x + map_extent(sx, -H(right), H(right), width),
//                    row = axis.y + (height - 1) - map_extent(sy, -H(up), H(up), height): the rule of debug_panels.hip
//   depth level      q = floor((depth + H_t) / (2 H_t) * 65535 + 0.5) clamped to 0 .. 65535; nearer is larger
//   stamp            the k x k square whose top-left is (column - k / 2, row - k / 2), clipped to the axis rectangle
//   visibility       at every pixel the point with the largest (q, point number n L + i) wins; it shows LUT[c],
//                    c = floor((v - c_lo) / (c_hi - c_lo) * 255 + 0.5) clamped to 0 .. 255; no point: the chrome stays
//   marker           (marker_x, frame.cursor, marker_z) projected likewise, stamped opaque on top, no depth test
// Point pass, one lane per point: a 64-bit atomicMax of ((q + 1) << 40) | point number into the word of every stamped
// pixel. A maximum does not depend on the order of its operands, so nothing depends on scheduling; because it only
// grows, a lane reads the word first and skips the atomic when its key cannot win (in a dense cloud hundreds of points
// meet on one pixel and almost all of them lose). Resolve pass, one lane per 16 pixels (three 16-byte vectors): the
// winner's value is read again and coloured, or the chrome is copied.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace gance_scatter3d {

constexpr int kMaxSide = 4096;
constexpr int kMaxSize = 64;
constexpr int kThreads = 256;
constexpr int kPointBits = 40;
constexpr int64_t kMaxPoints = (int64_t)1 << kPointBits;
constexpr int kMaxPointBlocks = 1 << 16;

struct Extents {
    double right, up, toward;  // H of the three view vectors
};

__host__ __device__ __forceinline__ double half_extent(const double* w) { return ((fabs(w[0]) + fabs(w[1])) + fabs(w[2])) / 2.0; }

// floor(t * scale + 0.5) of t = (v - lo) / (hi - lo), clamped to [low, high] (NaN: low)
__device__ __forceinline__ int map_clamped(double v, double lo, double hi, double scale, double low, double high) {
    const double t = (v - lo) / (hi - lo);
    const double u = t * scale;
    double r = floor(u + 0.5);
    if (!(r >= low)) r = low;
    if (r > high) r = high;
    return (int)r;
}

__device__ __forceinline__ int map_extent(double v, double lo, double hi, int extent) {
    return map_clamped(v, lo, hi, (double)(extent - 1), -32768.0, 32767.0);
}

__device__ __forceinline__ double dot3(const double* w, double ux, double uy, double uz) { return (w[0] * ux + w[1] * uy) + w[2] * uz; }

struct Projected {
    int column, row, level;  // column and row relative to the axis rectangle
};

__device__ __forceinline__ Projected project(const gance_debug_view3d& view, const Extents& h, double px, double py, double pz) {
    const double ux = (px - view.x_min) / (view.x_max - view.x_min) - 0.5;
    const double uy = (py - view.y_min) / (view.y_max - view.y_min) - 0.5;
    const double uz = (pz - view.z_min) / (view.z_max - view.z_min) - 0.5;
    const double sx = dot3(view.right, ux, uy, uz), sy = dot3(view.up, ux, uy, uz), depth = dot3(view.toward, ux, uy, uz);
    Projected p;
    p.column = map_extent(sx, -h.right, h.right, view.width);
    p.row = (view.height - 1) - map_extent(sy, -h.up, h.up, view.height);
    p.level = map_clamped(depth, -h.toward, h.toward, 65535.0, 0.0, 65535.0);
    return p;
}

// Element i of vector n; false if it is not finite
__device__ __forceinline__ bool read_value(const void* values, int dtype, int64_t index, double* value) {
    const double v = dtype == GANCE_DEBUG_F32 ? (double)((const float*)values)[index] : ((const double*)values)[index];
    *value = v;
    return isfinite(v);
}

// ---- point pass: keys[pixel] = max over the points that reach it of ((q + 1) << 40) | point number ---------------------
__global__ void __launch_bounds__(kThreads) scatter3d_points_kernel(gance_debug_view3d view, Extents h, int side, const void* __restrict__ values,
                                                                    int dtype, int64_t num_points, int64_t vector_length,
                                                                    int64_t vector_stride, unsigned long long* keys) {
    const int k = view.point_size;
    for (int64_t point = (int64_t)blockIdx.x * kThreads + threadIdx.x; point < num_points; point += (int64_t)gridDim.x * kThreads) {
        const int64_t n = point / vector_length, i = point - n * vector_length;
        double v;
        if (!read_value(values, dtype, n * vector_stride + i, &v)) continue;
        const Projected p = project(view, h, (double)i, (double)n, v);
        const unsigned long long key = ((unsigned long long)(p.level + 1) << kPointBits) | (unsigned long long)point;
        const int x_lo = max(p.column - k / 2, 0), x_hi = min(p.column - k / 2 + k, view.width);
        const int y_lo = max(p.row - k / 2, 0), y_hi = min(p.row - k / 2 + k, view.height);
        for (int y = y_lo; y < y_hi; ++y)
            for (int x = x_lo; x < x_hi; ++x) {
                unsigned long long* word = keys + (int64_t)(view.y + y) * side + (view.x + x);
                // (a stale, smaller value read here only costs an atomic that loses)
                if (__atomic_load_n(word, __ATOMIC_RELAXED) < key) atomicMax(word, key);
            }
    }
}

__device__ __forceinline__ void put_byte(uint4& vector, int byte, uint8_t value) {
    uint32_t* words = (uint32_t*)&vector;
    const int shift = 8 * (byte & 3);
    words[byte >> 2] = (words[byte >> 2] & ~(0xFFu << shift)) | ((uint32_t)value << shift);
}

// ---- resolve pass: one lane per 16 pixels of a row (48 bytes) ------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) scatter3d_resolve_kernel(const uint8_t* __restrict__ chrome, int side, double c_min, double c_max,
                                                                     const void* __restrict__ values, int dtype, int64_t vector_length,
                                                                     int64_t vector_stride, const uint8_t* __restrict__ lut,
                                                                     const unsigned long long* __restrict__ keys, uint8_t* __restrict__ out) {
    const int64_t group = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // 16 pixels
    if (group >= (int64_t)side * side / 16) return;
    const uint4* from = (const uint4*)(chrome + group * 48);
    uint4 bytes[3] = {from[0], from[1], from[2]};
    for (int pixel = 0; pixel < 16; ++pixel) {
        const unsigned long long key = keys[group * 16 + pixel];
        if (key == 0) continue;
        const int64_t point = (int64_t)(key & ((1ull << kPointBits) - 1));
        const int64_t n = point / vector_length, i = point - n * vector_length;
        double v;
        read_value(values, dtype, n * vector_stride + i, &v);
        const int c = map_clamped(v, c_min, c_max, 255.0, 0.0, 255.0);
        for (int channel = 0; channel < 3; ++channel) {
            const int byte = pixel * 3 + channel;
            put_byte(bytes[byte >> 4], byte & 15, lut[c * 3 + channel]);
        }
    }
    uint4* to = (uint4*)(out + group * 48);
    to[0] = bytes[0];
    to[1] = bytes[1];
    to[2] = bytes[2];
}

// ---- per frame: the template with the frame's marker; grid (side, batch), a row of one frame per workgroup -----------------
// The lane that copies a 16-byte vector also sets the marker's bytes inside it: no byte is written twice.
__global__ void __launch_bounds__(kThreads) scatter3d_frames_kernel(const uint8_t* __restrict__ pattern, gance_debug_view3d view, Extents h, int side,
                                                                    const gance_debug_frame* __restrict__ frames, uint8_t* __restrict__ out,
                                                                    int64_t out_frame_stride, int64_t out_row_stride) {
    const int row = blockIdx.x;
    const int64_t b = blockIdx.y;
    const double cursor = frames[b].cursor;
    int first_byte = 0, last_byte = 0;  // the marker's bytes [first, last) of this row
    if (isfinite(cursor)) {
        const Projected p = project(view, h, view.marker_x, cursor, view.marker_z);
        const int k = view.marker_size;
        const int x_lo = max(p.column - k / 2, 0), x_hi = min(p.column - k / 2 + k, view.width);
        const int y_lo = max(p.row - k / 2, 0), y_hi = min(p.row - k / 2 + k, view.height);
        if (row >= view.y + y_lo && row < view.y + y_hi && x_lo < x_hi) {
            first_byte = (view.x + x_lo) * 3;
            last_byte = (view.x + x_hi) * 3;
        }
    }
    const uint4* from = (const uint4*)(pattern + (int64_t)row * side * 3);
    uint4* to = (uint4*)(out + b * out_frame_stride + row * out_row_stride);
    const int vectors = side * 3 / 16;
    for (int i = threadIdx.x; i < vectors; i += kThreads) {
        uint4 bytes = from[i];
        const int lo = max(first_byte, 16 * i), hi = min(last_byte, 16 * i + 16);
        for (int byte = lo; byte < hi; ++byte) put_byte(bytes, byte - 16 * i, view.marker_rgb[byte % 3]);
        to[i] = bytes;
    }
}

static int fail(int code, const std::string& message) { return gance::set_last_error(code, message); }

static int invalid(const char* entry, const std::string& message) { return fail(GANCE_ERR_INVALID_ARGUMENT, std::string(entry) + ": " + message); }

static int check_side(const char* entry, int32_t side) {
    if (side < 16 || side > kMaxSide || side % 16 != 0)
        return invalid(entry, "side must be a multiple of 16 in [16, " + std::to_string(kMaxSide) + "], got " + std::to_string(side));
    return GANCE_OK;
}

static bool differ(double lo, double hi) { return std::isfinite(lo) && std::isfinite(hi) && lo != hi; }

static int check_view(const char* entry, const gance_debug_view3d& view, int32_t side) {
    if (view.width < 1 || view.height < 1 || view.x < 0 || view.y < 0 || view.x > side - view.width || view.y > side - view.height)
        return invalid(entry, "the axis rectangle (" + std::to_string(view.x) + ", " + std::to_string(view.y) + ", " + std::to_string(view.width) +
                                  ", " + std::to_string(view.height) + ") does not lie inside the panel");
    const struct {
        const char* name;
        double lo, hi;
    } limits[4] = {{"x", view.x_min, view.x_max}, {"y", view.y_min, view.y_max}, {"z", view.z_min, view.z_max}, {"colour", view.c_min, view.c_max}};
    for (const auto& pair : limits)
        if (!differ(pair.lo, pair.hi))
            return invalid(entry, std::string("the ") + pair.name + " limits must be finite and differ, got " + std::to_string(pair.lo) + " .. " +
                                      std::to_string(pair.hi));
    const struct {
        const char* name;
        const double* w;
    } vectors[3] = {{"right", view.right}, {"up", view.up}, {"toward", view.toward}};
    for (const auto& vector : vectors) {
        const double* w = vector.w;
        if (!std::isfinite(w[0]) || !std::isfinite(w[1]) || !std::isfinite(w[2]) || (w[0] == 0.0 && w[1] == 0.0 && w[2] == 0.0))
            return invalid(entry, std::string("the view vector `") + vector.name + "` must be finite and not all zero");
    }
    if (view.point_size < 1 || view.point_size > kMaxSize)
        return invalid(entry, "point_size must be in [1, " + std::to_string(kMaxSize) + "], got " + std::to_string(view.point_size));
    if (view.marker_size < 1 || view.marker_size > kMaxSize)
        return invalid(entry, "marker_size must be in [1, " + std::to_string(kMaxSize) + "], got " + std::to_string(view.marker_size));
    if (!std::isfinite(view.marker_x) || !std::isfinite(view.marker_z)) return invalid(entry, "the marker's x and z must be finite");
    return GANCE_OK;
}

static int no_device() {
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return fail(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    return GANCE_OK;
}

static Extents extents_of(const gance_debug_view3d& view) { return Extents{half_extent(view.right), half_extent(view.up), half_extent(view.toward)}; }

}  // namespace gance_scatter3d

extern "C" {

int gance_debug_scatter3d_u8(const uint8_t* d_chrome, int32_t side, const gance_debug_view3d* view, const void* d_values, int32_t dtype,
                             int64_t num_vectors, int64_t vector_length, int64_t vector_stride, const uint8_t* d_lut, uint64_t* d_keys,
                             uint8_t* d_template, void* stream) {
    using namespace gance_scatter3d;
    const char* entry = "gance_debug_scatter3d_u8";
    if (d_chrome == nullptr || view == nullptr || d_values == nullptr || d_lut == nullptr || d_keys == nullptr || d_template == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string("NULL argument to ") + entry);
    if (const int status = check_side(entry, side)) return status;
    if (dtype != GANCE_DEBUG_F32 && dtype != GANCE_DEBUG_F64)
        return invalid(entry, "values must be GANCE_DEBUG_F32 or GANCE_DEBUG_F64, got dtype " + std::to_string(dtype));
    if ((uintptr_t)d_chrome % 16 != 0 || (uintptr_t)d_template % 16 != 0 || (uintptr_t)d_keys % 8 != 0 ||
        (uintptr_t)d_values % (dtype == GANCE_DEBUG_F64 ? 8 : 4) != 0)
        return invalid(entry, "chrome and template must be 16-byte aligned, the keys 8-byte, the values to their element");
    if (num_vectors < 1 || vector_length < 1 || num_vectors > (kMaxPoints - 1) / vector_length)
        return invalid(entry, "num_vectors * vector_length must be in [1, 2^40), got " + std::to_string(num_vectors) + " * " +
                                  std::to_string(vector_length));
    if (vector_stride < vector_length) return invalid(entry, "vector_stride " + std::to_string(vector_stride) + " is smaller than a vector");
    if (const int status = check_view(entry, *view, side)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_template));  // launch where the template lives
    if (guard.status() != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));
    hipStream_t s = (hipStream_t)stream;
    const int64_t pixels = (int64_t)side * side, num_points = num_vectors * vector_length;
    hipError_t err = hipMemsetAsync(d_keys, 0, (size_t)pixels * sizeof(uint64_t), s);
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("scatter3d workspace: ") + hipGetErrorString(err));
    const Extents h = extents_of(*view);
    const int64_t point_blocks = (num_points + kThreads - 1) / kThreads;
    scatter3d_points_kernel<<<(unsigned)(point_blocks < kMaxPointBlocks ? point_blocks : kMaxPointBlocks), kThreads, 0, s>>>(
        *view, h, side, d_values, dtype, num_points, vector_length, vector_stride, (unsigned long long*)d_keys);
    scatter3d_resolve_kernel<<<(unsigned)((pixels / 16 + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        d_chrome, side, view->c_min, view->c_max, d_values, dtype, vector_length, vector_stride, d_lut, (const unsigned long long*)d_keys,
        d_template);
    err = hipGetLastError();
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("scatter3d launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

int gance_debug_draw_scatter3d_u8(const uint8_t* d_template, int32_t side, const gance_debug_view3d* view, const gance_debug_frame* d_frames,
                                  int32_t batch, uint8_t* d_out, int64_t out_frame_stride, int64_t out_row_stride, void* stream) {
    using namespace gance_scatter3d;
    const char* entry = "gance_debug_draw_scatter3d_u8";
    if (d_template == nullptr || view == nullptr || d_frames == nullptr || d_out == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string("NULL argument to ") + entry);
    if (batch < 1 || batch > 65535) return invalid(entry, "batch must be in [1, 65535], got " + std::to_string(batch));
    if (const int status = check_side(entry, side)) return status;
    if ((uintptr_t)d_out % 16 != 0 || out_row_stride % 16 != 0 || out_frame_stride % 16 != 0)
        return invalid(entry, "output and its strides must be 16-byte aligned");
    if (out_row_stride < (int64_t)side * 3 || out_frame_stride < (int64_t)(side - 1) * out_row_stride + (int64_t)side * 3)
        return invalid(entry, "output strides smaller than a panel");
    if ((uintptr_t)d_template % 16 != 0 || (uintptr_t)d_frames % 8 != 0) return invalid(entry, "template must be 16-byte and frames 8-byte aligned");
    if (const int status = check_view(entry, *view, side)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_out));  // launch where the frames live
    if (guard.status() != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));
    scatter3d_frames_kernel<<<dim3((unsigned)side, (unsigned)batch), kThreads, 0, (hipStream_t)stream>>>(
        d_template, *view, extents_of(*view), side, d_frames, d_out, out_frame_stride, out_row_stride);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("scatter3d launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

}  // extern "C"
