// Lossless stills: PNG files (8-bit RGB, no interlace) of uint8 frames in HBM: gance_png_encode_bounds /
// gance_png_encode_u8 of include/gance_hip.h. The replacement of PIL's Image.save(format="PNG") in
// gance/image_sources/still_image_common.py:19-28 and synthesize_images.py:188-191.
//
// The stages, their kernels and the launches of a call are in png_common.h, shared with the match-search encoder of
// png_lz.hip; this file is the literal-only encoder's two entries.

#include "png_common.h"

extern "C" {

int gance_png_encode_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes, uint64_t* out_capacity) {
    return gance_png::bounds_call("gance_png_encode_bounds", 0, batch, width, height, workspace_bytes, out_capacity);
}

int gance_png_encode_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, void* d_workspace, uint64_t workspace_bytes,
                        uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets, void* stream_ptr) {
    const auto nothing = [](hipStream_t, const gance_png::Layout&, unsigned, const uint8_t*, uint8_t*, int*, char*) {};
    return gance_png::encode_call("gance_png_encode_u8", "gance_png_encode_bounds", 0, nothing, d_frames, batch, width, height, d_workspace,
                                  workspace_bytes, d_out, out_capacity, d_offsets, stream_ptr);
}

}  // extern "C"
