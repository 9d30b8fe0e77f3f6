// Debug-video panels in HBM: gance_debug_place_panels_u8 and gance_debug_draw_panels_u8 of include/gance_hip.h.
//
// A debug frame is a row of square panels [side][P * side][3]. Image panels are placed by a strided row copy
// (16 bytes per lane); plot panels are a per-window chrome template (axes boxes, titles, labels, threshold lines:
// drawn once on the host) copied the same way, with the frame's marks rasterised on top.
//
// The rasterisation rule, all in integers once a value is mapped:
//   value -> pixel   column = axis.x + floor((v - x_min) / (x_max - x_min) * (width - 1) + 0.5)
//                    row    = axis.y + (height - 1) - floor((v - y_min) / (y_max - y_min) * (height - 1) + 0.5)
//                    in double, no contraction (this file is compiled with -ffp-contract=off), the floor clamped to
//                    [-32768, 32767]; a sample that is not finite is not drawn, nor is a segment that touches one
//   stamp            a mark of size k covers the k x k square whose top-left is (column - k / 2, row - k / 2)
//   line stepping    from (xa, ya) to (xb, yb): n = max(|dx|, |dy|) steps, step s at
//                    (xa + floor((2 s dx + n) / (2 n)), ya + floor((2 s dy + n) / (2 n))), each stamped
//   dash             a step is drawn iff floor_mod(column - axis.x, on + off) < on (the column of the step, not of the
//                    stamp's pixels); on = 0 means solid
//   blend            channel = (colour * a + channel * (255 - a) + 127) / 255 with a in 0 .. 255
//   clipping         a mark writes inside its axis rectangle only
// Marks are composited in table order. One workgroup owns one (frame, axis); a mark first sets its pixels in an LDS
// bit mask (atomic OR), then the mask is swept and every set pixel blended exactly once: overlaps inside one mark
// (a polyline crossing itself, stamps of neighbouring steps) cannot blend twice, and nothing depends on scheduling.
// Axis rectangles of one call are disjoint (checked), so workgroups never touch the same byte.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace gance_debug {

constexpr int kMaxSide = 4096;
constexpr int kMaxAxes = GANCE_DEBUG_MAX_AXES;
constexpr int kMaxMarks = GANCE_DEBUG_MAX_MARKS;
constexpr int kMaxMarkSize = 64;
constexpr int kThreads = 256;
constexpr int kMaskWords = 8192;  // 32 KiB of LDS: 64 rows of the widest axis, the whole axis up to 512 x 512

struct Tables {
    int32_t num_axes, num_marks;
    gance_debug_axis axes[kMaxAxes];
    gance_debug_mark marks[kMaxMarks];
};

// ---- placing panels ----------------------------------------------------------------------------------------------
// Panel of batch frame b <- src[(first_number + b) / divisor - src_base] ([side][side][3]); grid (side, batch).
__global__ void __launch_bounds__(kThreads) debug_place_kernel(const uint8_t* __restrict__ src, int side, int64_t first_number,
                                                               int divisor, int64_t src_base, uint8_t* __restrict__ out,
                                                               int64_t out_frame_stride, int64_t out_row_stride) {
    const int row = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int64_t source = (first_number + b) / divisor - src_base;
    const uint4* from = (const uint4*)(src + (source * side + row) * (int64_t)side * 3);
    uint4* to = (uint4*)(out + b * out_frame_stride + row * out_row_stride);
    const int vectors = side * 3 / 16;
    for (int i = threadIdx.x; i < vectors; i += kThreads) to[i] = from[i];
}

// ---- marks -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int map_extent(double v, double lo, double hi, int extent) {
    const double t = (v - lo) / (hi - lo);
    const double u = t * (double)(extent - 1);
    double r = floor(u + 0.5);
    if (!(r >= -32768.0)) r = -32768.0;
    if (r > 32767.0) r = 32767.0;
    return (int)r;
}

__device__ __forceinline__ int floor_div(int64_t a, int64_t b) {  // b > 0
    const int64_t q = a / b;
    return (int)(a % b < 0 ? q - 1 : q);
}

// Sample i of the series row `row`; false if it lies outside the series or is not finite
__device__ __forceinline__ bool read_sample(const gance_debug_mark& mark, int64_t row, int64_t i, double* value) {
    const int64_t index = row * mark.frame_stride + i;
    if (index < 0 || index >= mark.limit) return false;
    double v;
    if (mark.dtype == GANCE_DEBUG_F32) v = (double)((const float*)mark.data)[index];
    else if (mark.dtype == GANCE_DEBUG_F64) v = ((const double*)mark.data)[index];
    else v = (double)((const int32_t*)mark.data)[index];
    *value = v;
    return isfinite(v);
}

struct Band {
    int width, words_per_row, first_row, rows;  // rows [first_row, first_row + rows) of the axis rectangle
};

// The k x k stamp around (column, row), both relative to the axis rectangle, into the band's mask
__device__ __forceinline__ void stamp(uint32_t* mask, const Band& band, int column, int row, int k) {
    const int x_lo = max(column - k / 2, 0), x_hi = min(column - k / 2 + k, band.width);
    const int y_lo = max(row - k / 2, band.first_row), y_hi = min(row - k / 2 + k, band.first_row + band.rows);
    for (int y = y_lo; y < y_hi; ++y)
        for (int x = x_lo; x < x_hi; ++x) atomicOr(&mask[(y - band.first_row) * band.words_per_row + (x >> 5)], 1u << (x & 31));
}

__device__ __forceinline__ bool dash_on(const gance_debug_mark& mark, int column) {
    if (mark.dash_on <= 0) return true;
    const int period = mark.dash_on + mark.dash_off;
    int phase = column % period;
    if (phase < 0) phase += period;
    return phase < mark.dash_on;
}

// Pixels of `mark` on frame `frame` inside `band`, relative to the axis rectangle
__device__ void cover(const gance_debug_mark& mark, const gance_debug_axis& axis, const gance_debug_frame& frame, const Band& band,
                      uint32_t* mask) {
    const int tid = threadIdx.x;
    const int w = axis.width, h = axis.height;
    const int64_t row = frame.number / mark.frame_divisor;
    if (mark.kind == GANCE_DEBUG_MARK_CURSOR) {
        if (!isfinite(frame.cursor)) return;
        const int column = map_extent(frame.cursor, axis.x_min, axis.x_max, w);
        for (int y = band.first_row + tid; y < band.first_row + band.rows; y += kThreads) stamp(mask, band, column, y, mark.size);
        // (the stamps of neighbouring rows overlap for size > 1; the mask absorbs that)
        return;
    }
    if (mark.kind == GANCE_DEBUG_MARK_BAR) {
        double value;
        if (!read_sample(mark, row, 0, &value)) return;
        const int a = map_extent(0.0, axis.x_min, axis.x_max, w), b = map_extent(value, axis.x_min, axis.x_max, w);
        const int x_lo = max(min(a, b), 0), x_hi = min(max(a, b), w - 1);
        const int y_lo = max(h / 4, band.first_row), y_hi = min(h - h / 4, band.first_row + band.rows);
        for (int y = y_lo; y < y_hi; ++y)
            for (int x = x_lo + tid; x <= x_hi; x += kThreads) stamp(mask, band, x, y, 1);
        return;
    }
    if (mark.kind == GANCE_DEBUG_MARK_POINTS) {
        for (int i = tid; i < mark.count; i += kThreads) {
            double value;
            if (!read_sample(mark, row, i, &value)) continue;
            const int column = map_extent(mark.x_start + (double)i, axis.x_min, axis.x_max, w);
            const int y = (h - 1) - map_extent(value, axis.y_min, axis.y_max, h);
            stamp(mask, band, column, y, mark.size);
        }
        return;
    }
    // polyline: one lane per segment
    for (int i = tid; i + 1 < mark.count; i += kThreads) {
        double va, vb;
        if (!read_sample(mark, row, i, &va) || !read_sample(mark, row, i + 1, &vb)) continue;
        const int xa = map_extent(mark.x_start + (double)i, axis.x_min, axis.x_max, w);
        const int xb = map_extent(mark.x_start + (double)(i + 1), axis.x_min, axis.x_max, w);
        const int ya = (h - 1) - map_extent(va, axis.y_min, axis.y_max, h);
        const int yb = (h - 1) - map_extent(vb, axis.y_min, axis.y_max, h);
        const int dx = xb - xa, dy = yb - ya;
        const int n = max(abs(dx), abs(dy));
        if (n == 0) {
            if (dash_on(mark, xa)) stamp(mask, band, xa, ya, mark.size);
            continue;
        }
        for (int s = 0; s <= n; ++s) {
            const int x = xa + floor_div(2 * (int64_t)s * dx + n, 2 * (int64_t)n);
            const int y = ya + floor_div(2 * (int64_t)s * dy + n, 2 * (int64_t)n);
            if (dash_on(mark, x)) stamp(mask, band, x, y, mark.size);
        }
    }
}

// grid (num_axes, batch): the marks of one axis on one frame, in table order
__global__ void __launch_bounds__(kThreads) debug_marks_kernel(Tables tables, int side, const gance_debug_frame* __restrict__ frames,
                                                               uint8_t* __restrict__ out, int64_t out_frame_stride,
                                                               int64_t out_row_stride) {
    __shared__ uint32_t mask[kMaskWords];
    const int a = blockIdx.x;
    const int64_t b = blockIdx.y;
    const gance_debug_axis& axis = tables.axes[a];
    const gance_debug_frame frame = frames[b];
    if (frame.number < 0) return;
    uint8_t* panel = out + b * out_frame_stride;
    Band band;
    band.width = axis.width;
    band.words_per_row = (axis.width + 31) / 32;
    const int band_rows = kMaskWords / band.words_per_row;
    for (int m = 0; m < tables.num_marks; ++m) {
        const gance_debug_mark& mark = tables.marks[m];
        if (mark.axis != a || (frame.flags & mark.flag_mask) != mark.flag_value) continue;  // (uniform over the workgroup)
        const int alpha = mark.rgba[3];
        for (band.first_row = 0; band.first_row < axis.height; band.first_row += band_rows) {
            band.rows = min(band_rows, axis.height - band.first_row);
            const int words = band.rows * band.words_per_row;
            for (int i = threadIdx.x; i < words; i += kThreads) mask[i] = 0;
            __syncthreads();
            cover(mark, axis, frame, band, mask);
            __syncthreads();
            for (int i = threadIdx.x; i < words; i += kThreads) {
                uint32_t bits = mask[i];
                const int y = axis.y + band.first_row + i / band.words_per_row;
                const int x0 = axis.x + 32 * (i % band.words_per_row);
                while (bits) {
                    const int bit = __builtin_ctz(bits);
                    bits &= bits - 1;
                    uint8_t* pixel = panel + y * out_row_stride + (int64_t)(x0 + bit) * 3;
                    for (int c = 0; c < 3; ++c) pixel[c] = (uint8_t)((mark.rgba[c] * alpha + pixel[c] * (255 - alpha) + 127) / 255);
                }
            }
            __syncthreads();  // (the next mark of this axis may blend over these pixels)
        }
    }
}

static int fail(int code, const std::string& message) { return gance::set_last_error(code, message); }

// side, batch and the output pitches of both entries
static int check_output(const char* entry, int32_t side, int32_t batch, const uint8_t* d_out, int64_t out_frame_stride,
                        int64_t out_row_stride) {
    const std::string name(entry);
    if (d_out == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL output given to " + name);
    if (batch < 1 || batch > 65535) return fail(GANCE_ERR_INVALID_ARGUMENT, name + ": batch must be in [1, 65535]");
    if (side < 16 || side > kMaxSide || side % 16 != 0)
        return fail(GANCE_ERR_INVALID_ARGUMENT, name + ": side must be a multiple of 16 in [16, " + std::to_string(kMaxSide) + "], got " +
                                                    std::to_string(side));
    if ((uintptr_t)d_out % 16 != 0 || out_row_stride % 16 != 0 || out_frame_stride % 16 != 0)
        return fail(GANCE_ERR_INVALID_ARGUMENT, name + ": output and its strides must be 16-byte aligned");
    if (out_row_stride < (int64_t)side * 3 || out_frame_stride < (int64_t)(side - 1) * out_row_stride + (int64_t)side * 3)
        return fail(GANCE_ERR_INVALID_ARGUMENT, name + ": output strides smaller than a panel");
    return GANCE_OK;
}

static int no_device() {
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return fail(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    return GANCE_OK;
}

static int check_tables(const gance_debug_axis* axes, int32_t num_axes, const gance_debug_mark* marks, int32_t num_marks, int32_t side) {
    const std::string name = "gance_debug_draw_panels_u8: ";
    if (num_axes < 1 || num_axes > kMaxAxes) return fail(GANCE_ERR_INVALID_ARGUMENT, name + "1 .. " + std::to_string(kMaxAxes) + " axes");
    if (num_marks < 0 || num_marks > kMaxMarks) return fail(GANCE_ERR_INVALID_ARGUMENT, name + "0 .. " + std::to_string(kMaxMarks) + " marks");
    for (int a = 0; a < num_axes; ++a) {
        const gance_debug_axis& axis = axes[a];
        if (axis.width < 1 || axis.height < 1 || axis.x < 0 || axis.y < 0 || axis.x > side - axis.width || axis.y > side - axis.height)
            return fail(GANCE_ERR_INVALID_ARGUMENT, name + "axis " + std::to_string(a) + " does not lie inside the panel");
        if (!std::isfinite(axis.x_min) || !std::isfinite(axis.x_max) || !std::isfinite(axis.y_min) || !std::isfinite(axis.y_max) ||
            axis.x_min == axis.x_max || axis.y_min == axis.y_max)
            return fail(GANCE_ERR_INVALID_ARGUMENT, name + "axis " + std::to_string(a) + " needs finite limits that differ");
        for (int o = 0; o < a; ++o) {
            const gance_debug_axis& other = axes[o];
            if (axis.x < other.x + other.width && other.x < axis.x + axis.width && axis.y < other.y + other.height &&
                other.y < axis.y + axis.height)
                return fail(GANCE_ERR_INVALID_ARGUMENT, name + "axes " + std::to_string(o) + " and " + std::to_string(a) + " overlap");
        }
    }
    for (int m = 0; m < num_marks; ++m) {
        const gance_debug_mark& mark = marks[m];
        const std::string which = name + "mark " + std::to_string(m);
        if (mark.kind < GANCE_DEBUG_MARK_POINTS || mark.kind > GANCE_DEBUG_MARK_BAR) return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": unknown kind");
        if (mark.axis < 0 || mark.axis >= num_axes) return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": unknown axis");
        if (mark.size < 1 || mark.size > kMaxMarkSize)
            return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": size must be in [1, " + std::to_string(kMaxMarkSize) + "]");
        if (mark.frame_divisor < 1) return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": frame_divisor must be >= 1");
        if (mark.dash_on < 0 || mark.dash_off < 0 || (mark.dash_on > 0 && mark.dash_off < 1))
            return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": bad dash pattern");
        if (mark.kind == GANCE_DEBUG_MARK_CURSOR) continue;
        if (mark.dtype < GANCE_DEBUG_F32 || mark.dtype > GANCE_DEBUG_I32) return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": unknown dtype");
        if (mark.count < 0 || mark.limit < 0 || mark.frame_stride < 0 || !std::isfinite(mark.x_start))
            return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": negative count, limit or stride");
        if (mark.data == nullptr || (uintptr_t)mark.data % (mark.dtype == GANCE_DEBUG_F64 ? 8 : 4) != 0)
            return fail(GANCE_ERR_INVALID_ARGUMENT, which + ": series pointer NULL or unaligned");
    }
    return GANCE_OK;
}

}  // namespace gance_debug

extern "C" {

int gance_debug_place_panels_u8(const uint8_t* d_src, int32_t src_count, int32_t side, int64_t first_number, int32_t divisor,
                                int64_t src_base, int32_t batch, uint8_t* d_out, int64_t out_frame_stride, int64_t out_row_stride,
                                void* stream) {
    using namespace gance_debug;
    if (d_src == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL source given to gance_debug_place_panels_u8");
    if (const int status = check_output("gance_debug_place_panels_u8", side, batch, d_out, out_frame_stride, out_row_stride)) return status;
    if ((uintptr_t)d_src % 16 != 0) return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_debug_place_panels_u8: source must be 16-byte aligned");
    if (divisor < 1 || first_number < 0 || src_count < 1)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_debug_place_panels_u8: divisor and src_count must be >= 1, first_number >= 0");
    const int64_t lowest = first_number / divisor - src_base, highest = (first_number + batch - 1) / divisor - src_base;
    if (lowest < 0 || highest >= src_count)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_debug_place_panels_u8: frames read sources " + std::to_string(lowest) + " .. " +
                                                    std::to_string(highest) + " of " + std::to_string(src_count));
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_out));  // launch where the frames live
    if (guard.status() != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));
    debug_place_kernel<<<dim3((unsigned)side, (unsigned)batch), kThreads, 0, (hipStream_t)stream>>>(
        d_src, side, first_number, divisor, src_base, d_out, out_frame_stride, out_row_stride);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("debug panel launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

int gance_debug_draw_panels_u8(const uint8_t* d_chrome, int32_t side, const gance_debug_axis* axes, int32_t num_axes,
                               const gance_debug_mark* marks, int32_t num_marks, const gance_debug_frame* d_frames, int32_t batch,
                               uint8_t* d_out, int64_t out_frame_stride, int64_t out_row_stride, void* stream) {
    using namespace gance_debug;
    if (d_chrome == nullptr || axes == nullptr || d_frames == nullptr || (marks == nullptr && num_marks != 0))
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_debug_draw_panels_u8");
    if (const int status = check_output("gance_debug_draw_panels_u8", side, batch, d_out, out_frame_stride, out_row_stride)) return status;
    if ((uintptr_t)d_chrome % 16 != 0 || (uintptr_t)d_frames % 8 != 0)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_debug_draw_panels_u8: chrome must be 16-byte and frames 8-byte aligned");
    if (const int status = check_tables(axes, num_axes, marks, num_marks, side)) return status;
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_out));  // launch where the frames live
    if (guard.status() != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));
    Tables tables{};
    tables.num_axes = num_axes;
    tables.num_marks = num_marks;
    for (int a = 0; a < num_axes; ++a) tables.axes[a] = axes[a];
    for (int m = 0; m < num_marks; ++m) tables.marks[m] = marks[m];
    hipStream_t s = (hipStream_t)stream;
    // the chrome of every frame is source 0: a divisor larger than any frame number of the batch
    debug_place_kernel<<<dim3((unsigned)side, (unsigned)batch), kThreads, 0, s>>>(d_chrome, side, 0, 1 << 30, 0, d_out, out_frame_stride,
                                                                                out_row_stride);
    if (num_marks > 0)
        debug_marks_kernel<<<dim3((unsigned)num_axes, (unsigned)batch), kThreads, 0, s>>>(tables, side, d_frames, d_out, out_frame_stride,
                                                                                          out_row_stride);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("debug panel launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

}  // extern "C"
