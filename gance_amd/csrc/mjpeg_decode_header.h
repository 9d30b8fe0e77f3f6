// Host side of the Motion-JPEG decoder that reads a file's segments: gance_jpeg_parse_header (4:2:2 only, as the encoder
// writes) and gance_jpeg_parse_header_layouts (4:2:2, 4:2:0, 4:4:4 and grey) of include/gance_hip.h, and the table checks
// the decode entries repeat on the descriptions they are given. Host only, no device call. Included by mjpeg_decode.hip,
// and by tools/jpeg_header_check.hip, which runs the parser under the host sanitizers on cut and damaged headers.
// Every read is checked against the file's size first: a segment's length against the file, a table against its segment.
#ifndef GANCE_MJPEG_DECODE_HEADER_H
#define GANCE_MJPEG_DECODE_HEADER_H

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/gance_hip.h"
#include "mjpeg_tables.h"

namespace gance {
int set_last_error(int code, const std::string& message);
}  // namespace gance

namespace gance_mjpeg_decode {

using gance_mjpeg::natural_of_zigzag;

constexpr int kMaxSide = 8192;

// What a layout fixes: the luma sampling factors, and with them the MCU (8 * h by 8 * v pixels) and its blocks in
// order: h * v of Y in raster order, then Cb, Cr (colour), or the one Y block (grey).
struct LayoutShape {
    int components, h, v, blocks_per_mcu;
};
inline LayoutShape shape_of(int layout) {
    switch (layout) {
        case GANCE_JPEG_LAYOUT_420: return {3, 2, 2, 6};
        case GANCE_JPEG_LAYOUT_444: return {3, 1, 1, 3};
        case GANCE_JPEG_LAYOUT_GREY: return {1, 1, 1, 1};
        default: return {3, 2, 1, 4};
    }
}

inline int fail(const std::string& message) { return gance::set_last_error(GANCE_ERR_INVALID_ARGUMENT, message); }

// counts sum to at most 256, the code is not over-subscribed, DC symbols are categories 0..11
inline bool table_error(const uint8_t bits[16], const uint8_t* values, bool dc, std::string* why) {
    int count = 0, code = 0;
    for (int length = 1; length <= 16; ++length) {
        count += bits[length - 1];
        code += bits[length - 1];
        if (code > (1 << length)) return *why = "over-subscribed Huffman table", true;
        code <<= 1;
    }
    if (count > 256) return *why = "Huffman table with more than 256 codes", true;
    if (dc)
        for (int i = 0; i < count; ++i)
            if (values[i] > 11) return *why = "DC Huffman table with a category above 11", true;
    return false;
}

inline void annex_k_tables(gance_jpeg_info* info, int components) {
    using namespace gance_mjpeg;
    for (int c = 0; c < components; ++c) {
        const bool chroma = c > 0;
        std::memset(info->huff_values[c], 0, sizeof(info->huff_values[c]));
        std::memcpy(info->huff_bits[c][0], chroma ? kDcChromaBits : kDcLumaBits, 16);
        std::memcpy(info->huff_values[c][0], kDcValues, sizeof(kDcValues));
        std::memcpy(info->huff_bits[c][1], chroma ? kAcChromaBits : kAcLumaBits, 16);
        std::memcpy(info->huff_values[c][1], chroma ? kAcChromaValues : kAcLumaValues, sizeof(kAcLumaValues));
    }
}

inline std::string sampling_name(const int* sampling, int components) {
    std::string name;
    for (int c = 0; c < components; ++c)
        name += (c ? ", " : "") + std::to_string(sampling[c] >> 4) + "x" + std::to_string(sampling[c] & 15);
    return name;
}

// `layout` == nullptr: the strict entry, which takes 4:2:2 alone and says so in the words it always had. Otherwise the
// file's layout is stored there. Tables of components the file does not have stay zero.
inline int parse_header(const uint8_t* file, uint64_t size, gance_jpeg_info* info, int32_t* layout) {
    struct Huffman {
        bool defined = false;
        uint8_t bits[16] = {}, values[256] = {};
    };
    Huffman huffman[2][4];
    uint8_t quant[4][64];
    bool quant_defined[4] = {}, any_dht = false, have_frame = false;
    int quant_of[3] = {}, components = 3;
    std::memset(info, 0, sizeof(*info));
    if (layout != nullptr) *layout = GANCE_JPEG_LAYOUT_422;
    const std::string cut = "JPEG header cut short";
    if (size < 4 || file[0] != 0xFF || file[1] != 0xD8) return fail(size < 4 ? cut : "not a JPEG file (no SOI)");
    uint64_t at = 2;
    for (;;) {
        if (at + 4 > size) return fail(cut);
        if (file[at] != 0xFF) return fail("JPEG header: marker expected at byte " + std::to_string(at));
        const int marker = file[at + 1];
        if (marker == 0xFF) {  // fill byte
            ++at;
            continue;
        }
        if (marker == 0xD9) return fail("JPEG file without a scan");
        if (marker == 0x01 || (marker >= 0xD0 && marker <= 0xD7)) {  // no length
            at += 2;
            continue;
        }
        const uint64_t length = (uint64_t)file[at + 2] << 8 | file[at + 3];
        if (length < 2 || at + 2 + length > size) return fail(cut);
        const uint8_t* body = file + at + 4;
        const uint64_t body_bytes = length - 2;
        at += 2 + length;
        if (marker == 0xDB) {
            for (uint64_t i = 0; i < body_bytes;) {
                const int precision = body[i] >> 4, id = body[i] & 15;
                if (precision != 0) return fail("unsupported JPEG: 16-bit DQT");
                if (id > 3) return fail("JPEG header: quantisation table id " + std::to_string(id));
                if (i + 65 > body_bytes) return fail(cut);
                for (int z = 0; z < 64; ++z) quant[id][natural_of_zigzag(z)] = body[i + 1 + z];
                quant_defined[id] = true;
                i += 65;
            }
        } else if (marker == 0xC4) {
            for (uint64_t i = 0; i < body_bytes;) {
                const int cls = body[i] >> 4, id = body[i] & 15;
                if (cls > 1 || id > 3) return fail("JPEG header: Huffman table class " + std::to_string(cls) + " id " + std::to_string(id));
                if (i + 17 > body_bytes) return fail(cut);
                Huffman& table = huffman[cls][id];
                int count = 0;
                for (int k = 0; k < 16; ++k) count += body[i + 1 + k];
                std::string why;
                if (table_error(body + i + 1, nullptr, false, &why)) return fail("invalid JPEG: " + why);  // the counts alone
                if (i + 17 + count > body_bytes) return fail(cut);
                std::memcpy(table.bits, body + i + 1, 16);
                std::memset(table.values, 0, 256);
                std::memcpy(table.values, body + i + 17, count);
                if (table_error(table.bits, table.values, cls == 0, &why)) return fail("invalid JPEG: " + why);
                table.defined = any_dht = true;
                i += 17 + count;
            }
        } else if (marker == 0xC0) {
            if (have_frame) return fail("JPEG header: more than one SOF");
            if (body_bytes < 6) return fail(cut);
            if (body[0] != 8) return fail("unsupported JPEG: " + std::to_string(body[0]) + "-bit samples (12-bit samples are not baseline)");
            info->height = body[1] << 8 | body[2];
            info->width = body[3] << 8 | body[4];
            components = body[5];
            if (components == 1 && layout == nullptr) return fail("unsupported JPEG: grey (one component); only 4:2:2 colour is decoded");
            if (components != 3 && components != 1) return fail("unsupported JPEG: " + std::to_string(components) + " components");
            if (body_bytes < 6 + 3 * (uint64_t)components) return fail(cut);
            int sampling[3] = {};
            for (int c = 0; c < components; ++c) {
                sampling[c] = body[6 + 3 * c + 1];
                quant_of[c] = body[6 + 3 * c + 2];
                if (quant_of[c] > 3) return fail("JPEG header: quantisation table id " + std::to_string(quant_of[c]));
            }
            if (layout == nullptr) {
                if (sampling[1] != 0x11 || sampling[2] != 0x11 || sampling[0] != 0x21) {
                    const char* name = sampling[1] == 0x11 && sampling[2] == 0x11
                                           ? (sampling[0] == 0x22 ? "4:2:0" : (sampling[0] == 0x11 ? "4:4:4" : "this chroma sampling"))
                                           : "this chroma sampling";
                    return fail(std::string("unsupported JPEG: ") + name + "; only 4:2:2 (2x1, 1x1, 1x1) is decoded");
                }
            } else if (components == 1) {
                *layout = GANCE_JPEG_LAYOUT_GREY;  // one component: one block per MCU whatever its factors (T.81 A.2.2)
            } else {
                const bool chroma_1x1 = sampling[1] == 0x11 && sampling[2] == 0x11;
                if (chroma_1x1 && sampling[0] == 0x21) *layout = GANCE_JPEG_LAYOUT_422;
                else if (chroma_1x1 && sampling[0] == 0x22) *layout = GANCE_JPEG_LAYOUT_420;
                else if (chroma_1x1 && sampling[0] == 0x11) *layout = GANCE_JPEG_LAYOUT_444;
                else {
                    const char* name = !chroma_1x1 ? "" : (sampling[0] == 0x12 ? "4:4:0, " : (sampling[0] == 0x41 ? "4:1:1, " : ""));
                    return fail(std::string("unsupported JPEG: ") + name + "sampling factors " + sampling_name(sampling, 3) +
                                "; 4:2:2 (2x1), 4:2:0 (2x2) and 4:4:4 (1x1) with 1x1 chroma, and grey, are decoded");
                }
            }
            if (info->width < 1 || info->width > kMaxSide || info->height < 1 || info->height > kMaxSide)
                return fail("unsupported JPEG: " + std::to_string(info->width) + " x " + std::to_string(info->height) +
                            ", width and height must be in [1, " + std::to_string(kMaxSide) + "]");
            have_frame = true;
        } else if (marker >= 0xC1 && marker <= 0xCF && marker != 0xC8 && marker != 0xCC) {
            return fail(std::string("unsupported JPEG: ") + (marker == 0xC2 ? "progressive" : (marker == 0xC1 ? "extended sequential" : "not baseline")) +
                        " (SOF" + std::to_string(marker - 0xC0) + "); only baseline SOF0 is decoded");
        } else if (marker == 0xDD) {
            if (body_bytes < 2) return fail(cut);
            info->restart_interval = body[0] << 8 | body[1];
        } else if (marker == 0xDA) {
            if (!have_frame) return fail("JPEG header: SOS before SOF");
            if (body_bytes < 1) return fail(cut);
            if (body[0] != components)
                return fail("unsupported JPEG: more than one scan (a scan of " + std::to_string(body[0]) + " of the " + std::to_string(components) +
                            " components)");
            const uint64_t tail = 1 + 2 * (uint64_t)components;  // Ss, Se, Ah/Al follow the components' table ids
            if (body_bytes < tail + 3) return fail(cut);
            if (body[tail] != 0 || body[tail + 1] != 63 || body[tail + 2] != 0)
                return fail("unsupported JPEG: a scan that is not baseline (spectral selection or approximation)");
            if (!any_dht) annex_k_tables(info, components);
            info->has_huffman_tables = any_dht;
            for (int c = 0; c < components; ++c) {
                const int dc = body[2 + 2 * c] >> 4, ac = body[2 + 2 * c] & 15;
                if (dc > 3 || ac > 3) return fail("JPEG header: Huffman table id in SOS");
                if (any_dht) {
                    if (!huffman[0][dc].defined || !huffman[1][ac].defined) return fail("invalid JPEG: the scan uses a Huffman table the file does not define");
                    std::memcpy(info->huff_bits[c][0], huffman[0][dc].bits, 16);
                    std::memcpy(info->huff_values[c][0], huffman[0][dc].values, 256);
                    std::memcpy(info->huff_bits[c][1], huffman[1][ac].bits, 16);
                    std::memcpy(info->huff_values[c][1], huffman[1][ac].values, 256);
                }
                if (!quant_defined[quant_of[c]]) return fail("invalid JPEG: a component uses a quantisation table the file does not define");
                std::memcpy(info->quant[c], quant[quant_of[c]], 64);
            }
            info->scan_offset = at;
            info->scan_bytes = size - at;
            return GANCE_OK;
        }
        // APPn, COM and anything else with a length: skipped
    }
}

}  // namespace gance_mjpeg_decode

// The two parsing entries are defined here, so that the sanitizer check runs exactly the code the library exports: one
// translation unit of a binary includes this header.
extern "C" {

int gance_jpeg_parse_header(const uint8_t* file, uint64_t file_bytes, gance_jpeg_info* info) {
    using namespace gance_mjpeg_decode;
    if (file == nullptr || info == nullptr) return fail("NULL argument to gance_jpeg_parse_header");
    return parse_header(file, file_bytes, info, nullptr);
}

int gance_jpeg_parse_header_layouts(const uint8_t* file, uint64_t file_bytes, gance_jpeg_frame_info* info) {
    using namespace gance_mjpeg_decode;
    if (file == nullptr || info == nullptr) return fail("NULL argument to gance_jpeg_parse_header_layouts");
    info->reserved = 0;
    return parse_header(file, file_bytes, &info->info, &info->layout);
}

}  // extern "C"

#endif
