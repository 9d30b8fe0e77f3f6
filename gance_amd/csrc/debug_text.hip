// Per-frame text on a debug panel in HBM: gance_debug_draw_text_u8 and gance_debug_font_columns of include/gance_hip.h.
//
// Every other piece of text of a plot panel is drawn once per window on the host into the chrome template. A title that
// changes on every frame ("... frame: 3, step: 417") is drawn here instead, on top of what gance_debug_draw_panels_u8 left:
// one short string per frame goes to HBM, not one template per frame.
//
// The rule is gance_amd/debug_video/font.py::draw_text:
//   string     the bytes d_text[b * text_stride ...] up to the first NUL, or all text_stride bytes; a byte outside
//              32 .. 126 is drawn as '?'
//   placement  glyph i covers the columns x + i * 6 * scale ... + 5 * scale - 1 (one empty glyph column between glyphs)
//              and the rows y ... y + 7 * scale - 1; a pixel is set to the colour, opaque, iff its glyph bit is set
//              (bit 0 of a column byte = top row)
//   clipping   to the panel and to the columns [x, x + max_width); nothing else is written (no background fill)
// One workgroup owns one frame: it stages the frame's string in LDS, finds its length once, then sweeps the box. Byte
// stores only; a pixel is written by exactly one lane.

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/gance_hip.h"
#include "debug_font.h"
#include "kernels.h"

namespace gance_debug_text {

constexpr int kMaxSide = 4096;
constexpr int kMaxTextStride = 256;
constexpr int kMaxScale = 64;
constexpr int kThreads = 256;
constexpr int kGlyphWidth = GANCE_DEBUG_FONT_GLYPH_WIDTH, kGlyphHeight = GANCE_DEBUG_FONT_GLYPH_HEIGHT;
constexpr int kAdvance = GANCE_DEBUG_FONT_ADVANCE;

static const uint8_t kHostColumns[GANCE_DEBUG_FONT_BYTES] = GANCE_DEBUG_FONT_COLUMNS;
__constant__ uint8_t kDeviceColumns[GANCE_DEBUG_FONT_BYTES] = GANCE_DEBUG_FONT_COLUMNS;

// grid (batch): the string of frame blockIdx.x
__global__ void __launch_bounds__(kThreads) debug_text_kernel(const uint8_t* __restrict__ text, int text_stride, int x, int y,
                                                              int max_width, int scale, uint32_t rgb, int side,
                                                              uint8_t* __restrict__ out, int64_t out_frame_stride,
                                                              int64_t out_row_stride) {
    __shared__ uint8_t glyphs[kMaxTextStride];  // glyph numbers (code - 32), '?' for what the font does not have
    __shared__ int length;
    const int64_t b = blockIdx.x;
    const uint8_t* string = text + b * text_stride;
    if (threadIdx.x == 0) length = text_stride;
    __syncthreads();
    for (int i = threadIdx.x; i < text_stride; i += kThreads) {  // (text_stride <= 256: one pass)
        const int code = string[i];
        if (code == 0) atomicMin(&length, i);
        glyphs[i] = (uint8_t)((code >= GANCE_DEBUG_FONT_FIRST && code <= GANCE_DEBUG_FONT_LAST ? code : '?') - GANCE_DEBUG_FONT_FIRST);
    }
    __syncthreads();
    const int count = length;
    if (count == 0) return;
    // the box: the text's own extent, clipped to max_width and to the panel (x, y in [0, side): both stay >= 1)
    const int cell = kAdvance * scale;
    const int text_width = (count * kAdvance - 1) * scale;
    const int width = min(min(text_width, max_width), side - x);
    const int height = min(kGlyphHeight * scale, side - y);
    uint8_t* panel = out + b * out_frame_stride;
    const uint8_t red = (uint8_t)(rgb & 0xFF), green = (uint8_t)((rgb >> 8) & 0xFF), blue = (uint8_t)((rgb >> 16) & 0xFF);
    for (int p = threadIdx.x; p < width * height; p += kThreads) {
        const int row = p / width, column = p % width;
        const int glyph_column = (column % cell) / scale;
        if (glyph_column >= kGlyphWidth) continue;  // the gap between glyphs
        const int bits = kDeviceColumns[glyphs[column / cell] * kGlyphWidth + glyph_column];
        if (!((bits >> (row / scale)) & 1)) continue;
        uint8_t* pixel = panel + (int64_t)(y + row) * out_row_stride + (int64_t)(x + column) * 3;
        pixel[0] = red;
        pixel[1] = green;
        pixel[2] = blue;
    }
}

static int fail(const std::string& message) {
    return gance::set_last_error(GANCE_ERR_INVALID_ARGUMENT, "gance_debug_draw_text_u8: " + message);
}

}  // namespace gance_debug_text

extern "C" {

int gance_debug_font_columns(uint8_t* h_out, uint64_t count) {
    if (h_out == nullptr || count != (uint64_t)GANCE_DEBUG_FONT_BYTES)
        return gance::set_last_error(GANCE_ERR_INVALID_ARGUMENT,
                                     "gance_debug_font_columns: the font has " + std::to_string(GANCE_DEBUG_FONT_BYTES) + " column bytes");
    std::memcpy(h_out, gance_debug_text::kHostColumns, count);
    return GANCE_OK;
}

int gance_debug_draw_text_u8(const uint8_t* d_text, int32_t text_stride, int32_t x, int32_t y, int32_t max_width, int32_t scale,
                             uint32_t rgb, int32_t side, int32_t batch, uint8_t* d_out, int64_t out_frame_stride,
                             int64_t out_row_stride, void* stream) {
    using namespace gance_debug_text;
    if (d_text == nullptr || d_out == nullptr) return fail("NULL text or output");
    if (batch < 1) return fail("batch must be >= 1, got " + std::to_string(batch));
    if (side < 16 || side > kMaxSide || side % 16 != 0)
        return fail("side must be a multiple of 16 in [16, " + std::to_string(kMaxSide) + "], got " + std::to_string(side));
    if ((uintptr_t)d_out % 16 != 0 || out_row_stride % 16 != 0 || out_frame_stride % 16 != 0)
        return fail("output and its strides must be 16-byte aligned");
    if (out_row_stride < (int64_t)side * 3 || out_frame_stride < (int64_t)(side - 1) * out_row_stride + (int64_t)side * 3)
        return fail("output strides smaller than a panel");
    if (text_stride < 1 || text_stride > kMaxTextStride)
        return fail("text_stride must be in [1, " + std::to_string(kMaxTextStride) + "], got " + std::to_string(text_stride));
    if (scale < 1 || scale > kMaxScale) return fail("scale must be in [1, " + std::to_string(kMaxScale) + "], got " + std::to_string(scale));
    if (max_width < 1) return fail("max_width must be >= 1, got " + std::to_string(max_width));
    if (x < 0 || x >= side || y < 0 || y >= side)
        return fail("(x, y) = (" + std::to_string(x) + ", " + std::to_string(y) + ") lies outside the panel");
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return gance::set_last_error(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    gance::DeviceGuard guard(gance::device_of_pointer(d_out));  // launch where the frames live
    if (guard.status() != hipSuccess)
        return gance::set_last_error(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));
    debug_text_kernel<<<dim3((unsigned)batch), kThreads, 0, (hipStream_t)stream>>>(d_text, text_stride, x, y, max_width, scale, rgb, side,
                                                                                  d_out, out_frame_stride, out_row_stride);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return gance::set_last_error(GANCE_ERR_HIP, std::string("debug text launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

}  // extern "C"
