// Baseline JPEG decoder for frames in HBM: gance_jpeg_parse_header / gance_jpeg_decode_bounds / gance_jpeg_decode_u8 of
// include/gance_hip.h (4:2:2 only, the reverse of mjpeg.hip) and gance_jpeg_parse_header_layouts /
// gance_jpeg_decode_layouts_bounds / gance_jpeg_decode_layouts_u8 (the same code for four layouts). Input: baseline
// sequential JFIF (SOF0, 8 bit), one interleaved scan of three components sampled 2x1 / 1x1 / 1x1 (4:2:2), 2x2 / 1x1 / 1x1
// (4:2:0) or 1x1 / 1x1 / 1x1 (4:4:4), or of one component (grey), any 8-bit DQT, any DHT or none (then the Annex K tables),
// any DRI or none, width and height in [1, 8192]; all frames of a call of one size and layout. Output: uint8
// [batch][height][width][3] RGB (grey: three equal channels), equal to libjpeg's default decode:
//
//   entropy decode      jdhuff.c decode_mcu: DC difference and AC run/size symbols with EXTEND; 0xFF 0x00 reads as 0xFF; the
//                       DC predictors restart with every restart segment
//   dequantise + IDCT   jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, columns then rows, the sample saturated
//                       to 0..255 as libjpeg-turbo's SIMD islow does (jidctint-sse2 / -avx2 / -neon pack with saturation;
//                       the C fallback's range-limit table wraps past +-512 instead: see DESIGN.md section 9 item 9)
//   chroma upsampling   jdsample.c over the component's true size: h2v1_fancy_upsample (4:2:2), h2v2_fancy_upsample (4:2:0),
//                       replication for both when the chroma width ceil(W / 2) is at most 2, none for 4:4:4
//   colour              jdcolor.c ycc_rgb_convert: 16-bit fixed point, arithmetic shifts, clamped
//
// Four launches on the caller's stream, no atomics on pixels, every frame independent of the others:
//   1. mjpeg_marker_scan_kernel   one workgroup per frame: the RSTn markers of its entropy-coded data compacted in order
//                                 into marker positions, the end of the data (EOI), and the frame's status when the
//                                 marker count or sequence is wrong (such a frame is not decoded)
//   2. mjpeg_entropy_kernel<n>    (n = 4, 6, 3 or 1 blocks per MCU: the layout) one thread per restart segment: Huffman
//                                 decode through a 9-bit look-ahead table in LDS (longer codes by the canonical maxcode
//                                 walk), int16 coefficients in natural order staged in a private LDS slot and written as
//                                 whole 128-byte blocks
//   3. mjpeg_idct_kernel          one thread per 8x8 block: dequantise, IDCT, range limit -> Y, Cb, Cr planes
//   4. mjpeg_colour_kernel<l>     (l = the layout) one thread per 16 pixels of a row: chroma upsampling across block
//                                 edges, colour, RGB
// Bounds: every read of compressed bytes lies inside the frame's scan range [scan_begin, scan_begin + scan_bytes), every
// coefficient index is below 64, a segment decodes at most its own MCUs, and a code that is not in the table ends the
// segment. The Huffman look-up tables are built on the host once per distinct set of tables of a call.

#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gance_hip.h"
#include "kernels.h"
#include "mjpeg_decode_header.h"
#include "mjpeg_tables.h"

namespace gance_mjpeg_decode {

constexpr int kLookBits = 9;
constexpr int kScanThreads = 256;
constexpr int kScanChunk = 16;  // bytes per thread and tile of the marker scan
constexpr int kEntropyThreads = 64;

// Decoder view of one Huffman table (jdhuff.c jpeg_make_d_derived_tbl)
struct DeviceTable {
    uint16_t fast[1 << kLookBits];  // by the next 9 bits: (code length << 8) | symbol; 0 = a longer code, or none
    int32_t maxcode[17];            // [l] the largest code of length l, -1 = no code of that length
    int32_t valoff[17];             // code c of length l is values[valoff[l] + c]
    uint8_t values[256];
};
struct alignas(16) TableSet {
    DeviceTable huff[3][2];  // [component][0 = DC, 1 = AC]
    uint16_t quant[3][64];   // natural order
};
struct alignas(16) FrameDesc {
    int64_t scan_begin;  // of the entropy-coded data inside d_data
    int32_t scan_bytes;
    int32_t restart_interval;
    int32_t segments;     // ceil(MCUs / restart_interval), 1 without restart markers
    int32_t marker_base;  // of this frame's segments - 1 entries of marker_pos
    int32_t table_set;
    int32_t reserved;
};

// ---- sizes -------------------------------------------------------------------------------------------------------
struct Layout {
    LayoutShape shape;
    int64_t mcu_cols, mcu_rows, mcus;  // per frame; an MCU is 8 * shape.h by 8 * shape.v pixels
    // Rows of the planes are `stride` bytes apart: the blocks' own width where the colour kernel reads 8 bytes per 16
    // pixels (4:2:2 and 4:2:0 chroma) or the width is a multiple of 16 anyway, rounded up to 16 where it reads 16 bytes
    // per 16 pixels of a plane that is a whole number of 8-wide blocks (4:4:4 and grey).
    int64_t luma_stride, luma_rows, chroma_stride, chroma_rows;
    int64_t params_bytes, marker_bytes, end_bytes, coef_bytes, luma_bytes, chroma_bytes, workspace_bytes;
    int64_t max_markers;
};

static int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

static Layout layout_of(int64_t batch, int64_t width, int64_t height, int layout) {
    Layout l{};
    l.shape = shape_of(layout);
    l.mcu_cols = (width + 8 * l.shape.h - 1) / (8 * l.shape.h);
    l.mcu_rows = (height + 8 * l.shape.v - 1) / (8 * l.shape.v);
    l.mcus = l.mcu_cols * l.mcu_rows;
    l.luma_stride = round16(l.mcu_cols * 8 * l.shape.h);
    l.luma_rows = l.mcu_rows * 8 * l.shape.v;
    l.chroma_stride = layout == GANCE_JPEG_LAYOUT_444 ? l.luma_stride : l.mcu_cols * 8;
    l.chroma_rows = l.mcu_rows * 8;
    l.max_markers = batch * (l.mcus - 1);  // a restart interval of one MCU
    l.params_bytes = round16(batch * (int64_t)sizeof(FrameDesc)) + batch * (int64_t)sizeof(TableSet);
    l.marker_bytes = round16(l.max_markers * 4);
    l.end_bytes = round16(batch * 4);
    l.coef_bytes = batch * l.mcus * l.shape.blocks_per_mcu * 64 * 2;
    l.luma_bytes = batch * l.luma_rows * l.luma_stride;
    l.chroma_bytes = l.shape.components == 3 ? batch * l.chroma_rows * l.chroma_stride : 0;
    l.workspace_bytes = l.params_bytes + l.marker_bytes + l.end_bytes + l.coef_bytes + l.luma_bytes + 2 * l.chroma_bytes;
    return l;
}

// ---- 1. marker scan ----------------------------------------------------------------------------------------------
template <typename T>
__device__ T block_exclusive_scan(T value, T* scratch, T* total) {
    const int tid = threadIdx.x;
    scratch[tid] = value;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const T add = tid >= d ? scratch[tid - d] : 0;
        __syncthreads();
        scratch[tid] += add;
        __syncthreads();
    }
    const T inclusive = scratch[tid];
    *total = scratch[kScanThreads - 1];
    __syncthreads();
    return inclusive - value;
}

// One workgroup per frame. Inside entropy-coded data 0xFF is followed by 0x00 (a stuffed data byte), 0xFF (fill), 0xD0..0xD7
// (RSTn) or another marker, which ends the data (EOI). marker_pos receives the positions of the first segments - 1 RSTn
// in order, scan_end the end of the data, or -1 for a frame that is not decoded; status the reason.
__global__ void __launch_bounds__(kScanThreads) mjpeg_marker_scan_kernel(const uint8_t* __restrict__ data, const FrameDesc* __restrict__ frames,
                                                                         int32_t* __restrict__ marker_pos, int32_t* __restrict__ scan_end,
                                                                         int32_t* __restrict__ status) {
    __shared__ int scratch[kScanThreads];
    __shared__ int s_end, s_bad;
    const int frame = blockIdx.x, tid = threadIdx.x;
    const FrameDesc f = frames[frame];
    const uint8_t* scan = data + f.scan_begin;
    const int n = f.scan_bytes, expected = f.segments - 1;
    if (tid == 0) s_end = n, s_bad = 0;
    __syncthreads();
    int carry = 0;
    for (int base = 0; base < n; base += kScanThreads * kScanChunk) {
        const int p0 = base + tid * kScanChunk;
        uint8_t b[kScanChunk + 1];
        if (p0 + kScanChunk + 1 <= n) {
#pragma unroll
            for (int i = 0; i < kScanChunk / 4; ++i) {
                uint32_t w;
                __builtin_memcpy(&w, scan + p0 + 4 * i, 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w >> (8 * j));
            }
            b[kScanChunk] = scan[p0 + kScanChunk];
        } else {
#pragma unroll
            for (int j = 0; j <= kScanChunk; ++j) b[j] = p0 + j < n ? scan[p0 + j] : 0;
        }
        int count = 0, end = n;
        uint32_t restarts = 0;
#pragma unroll
        for (int j = 0; j < kScanChunk; ++j) {
            const int v = b[j + 1];  // 0 past the end: a last byte 0xFF is no marker
            if (b[j] != 0xFF || v == 0 || v == 0xFF) continue;
            if (v >= 0xD0 && v <= 0xD7) restarts |= 1u << j, ++count;
            else end = min(end, p0 + j);
        }
        if (!__syncthreads_or(count | (end < n))) continue;
        int sum;
        int index = carry + block_exclusive_scan(count, scratch, &sum);
#pragma unroll
        for (int j = 0; j < kScanChunk; ++j) {
            if (!(restarts >> j & 1)) continue;
            if (index < expected) {
                marker_pos[f.marker_base + index] = p0 + j;
                if (b[j + 1] != 0xD0 + (index & 7)) s_bad = 1;
            }
            ++index;
        }
        if (end < n) atomicMin(&s_end, end);
        carry += sum;
    }
    __syncthreads();
    if (tid == 0) {
        int reason = GANCE_JPEG_OK;
        // fewer markers than the picture needs and no EOI: the data stops before the picture does
        if (carry != expected) reason = (carry < expected && s_end == n) ? GANCE_JPEG_TRUNCATED : GANCE_JPEG_MARKER_MISMATCH;
        else if (s_bad) reason = GANCE_JPEG_MARKER_MISMATCH;
        status[frame] = reason;
        scan_end[frame] = reason == GANCE_JPEG_OK ? s_end : -1;
    }
}

// ---- 2. entropy decode ---------------------------------------------------------------------------------------------
// Bits of one restart segment [pos, end) of `p`, MSB first in `acc`. Past the end zero bits are appended and counted in
// `pad`: the segment was cut short iff more bits were taken than it held (bits < pad).
struct BitReader {
    const uint8_t* p;
    int pos, end;
    uint64_t acc = 0;
    int bits = 0, pad = 0;
    __device__ BitReader(const uint8_t* data, int first, int last) : p(data), pos(first), end(last) {}
    // at least 32 bits afterwards (call with bits <= 32)
    __device__ __forceinline__ void refill() {
        if (pos + 4 <= end) {
            uint32_t w;
            __builtin_memcpy(&w, p + pos, 4);
            const uint32_t inverted = ~w;
            if (((inverted - 0x01010101u) & ~inverted & 0x80808080u) == 0) {  // no byte is 0xFF
                acc |= (uint64_t)__builtin_bswap32(w) << (32 - bits);
                bits += 32;
                pos += 4;
                return;
            }
        }
        while (bits <= 56) {
            uint32_t b = 0;
            if (pos < end) {
                b = p[pos];
                if (b != 0xFF) ++pos;
                else if (pos + 1 < end && p[pos + 1] == 0) pos += 2;
                else pos = end, b = 0, pad += 8;  // fill bytes or a cut stuffing pair: nothing more to read
            } else {
                pad += 8;
            }
            acc |= (uint64_t)b << (56 - bits);
            bits += 8;
        }
    }
    __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)(acc >> (64 - n)); }  // 1 <= n <= 32
    __device__ __forceinline__ void skip(int n) { acc <<= n, bits -= n; }
    __device__ __forceinline__ bool overrun() const { return bits < pad; }
};

// The next symbol (with at least 16 bits in the reader), or -1 for a code that is not in the table
__device__ __forceinline__ int decode_symbol(BitReader& reader, const uint16_t* __restrict__ fast, const DeviceTable& table) {
    const uint32_t entry = fast[reader.peek(kLookBits)];
    if (entry != 0) {
        reader.skip((int)(entry >> 8));
        return (int)(entry & 0xFF);
    }
    const int code16 = (int)reader.peek(16);
    for (int length = kLookBits + 1; length <= 16; ++length) {
        const int code = code16 >> (16 - length);
        if (code <= table.maxcode[length]) {
            const int index = table.valoff[length] + code;
            if (index < 0 || index > 255) return -1;
            reader.skip(length);
            return table.values[index];
        }
    }
    return -1;
}

// jdhuff.c HUFF_EXTEND: the `size`-bit field `value` as a signed coefficient
__device__ __forceinline__ int extend(int value, int size) { return value < (1 << (size - 1)) ? value - (1 << size) + 1 : value; }

// grid (ceil(max segments / 64), batch), one wave per workgroup. coef: [frame][mcu][kBlocks][64] int16, natural order.
// kBlocks is the layout's block list, fixed when the kernel is compiled, so that the symbol loop carries no test of the
// layout: 1 (grey: Y), 3 (4:4:4: Y, Cb, Cr), 4 (4:2:2: Y, Y, Cb, Cr) or 6 (4:2:0: four Y, Cb, Cr). Block k belongs to
// component 0 while k < kBlocks - 2 (every block of grey), then to component 1 and 2. Only the 2 * components Huffman
// tables the layout has are loaded or read.
template <int kBlocks>
__global__ void __launch_bounds__(kEntropyThreads) mjpeg_entropy_kernel(const uint8_t* __restrict__ data, const FrameDesc* __restrict__ frames,
                                                                        const TableSet* __restrict__ sets, const int32_t* __restrict__ marker_pos,
                                                                        const int32_t* __restrict__ scan_end, int32_t* __restrict__ status,
                                                                        int16_t* __restrict__ coef, int mcus) {
    constexpr int kComponents = kBlocks == 1 ? 1 : 3, kLumaBlocks = kBlocks == 1 ? 1 : kBlocks - 2;
    __shared__ uint16_t fast[2 * kComponents][1 << kLookBits];
    __shared__ uint32_t slots[32 * kEntropyThreads];  // word w of thread t's block at [w * 64 + t]: no bank conflicts
    __shared__ uint8_t natural[64];
    const int frame = blockIdx.y, tid = threadIdx.x;
    const FrameDesc f = frames[frame];
    const int frame_end = scan_end[frame];
    if ((int)blockIdx.x * kEntropyThreads >= f.segments || frame_end < 0) return;
    const TableSet& set = sets[f.table_set];
    for (int i = tid; i < 2 * kComponents * 256; i += kEntropyThreads) {
        const int t = i >> 8;
        ((uint32_t*)fast[t])[i & 255] = ((const uint32_t*)set.huff[t >> 1][t & 1].fast)[i & 255];
    }
    for (int i = tid; i < 32 * kEntropyThreads; i += kEntropyThreads) slots[i] = 0;
    natural[tid] = (uint8_t)natural_of_zigzag(tid);
    __syncthreads();
    const int segment = blockIdx.x * kEntropyThreads + tid;
    if (segment >= f.segments) return;

    const int* markers = marker_pos + f.marker_base;
    int last = segment == f.segments - 1 ? frame_end : markers[segment];
    int first = segment == 0 ? 0 : markers[segment - 1] + 2;
    last = max(0, min(last, f.scan_bytes));
    first = max(0, min(first, last));
    const int mcu_begin = f.restart_interval > 0 ? segment * f.restart_interval : 0;
    const int mcu_end = f.restart_interval > 0 ? min(mcus, mcu_begin + f.restart_interval) : mcus;

    BitReader reader(data + f.scan_begin, first, last);
    int16_t* slot = (int16_t*)slots;
    int predictor[kComponents] = {};
    int reason = GANCE_JPEG_OK;
    for (int mcu = mcu_begin; mcu < mcu_end && reason == GANCE_JPEG_OK; ++mcu) {
        for (int kind = 0; kind < kBlocks && reason == GANCE_JPEG_OK; ++kind) {
            const int c = kind < kLumaBlocks ? 0 : kind - kLumaBlocks + 1;
            if (reader.bits <= 32) reader.refill();
            int symbol = decode_symbol(reader, fast[2 * c], set.huff[c][0]);
            if (symbol < 0 || symbol > 15) {
                reason = GANCE_JPEG_INVALID_CODE;
                break;
            }
            if (symbol > 0) {
                const int value = (int)reader.peek(symbol);
                reader.skip(symbol);
                predictor[c] += extend(value, symbol);
            }
            slot[tid * 2] = (int16_t)predictor[c];
            for (int k = 1; k < 64;) {
                if (reader.bits <= 32) reader.refill();
                symbol = decode_symbol(reader, fast[2 * c + 1], set.huff[c][1]);
                if (symbol < 0) {
                    reason = GANCE_JPEG_INVALID_CODE;
                    break;
                }
                const int run = symbol >> 4, size = symbol & 15;
                if (size == 0) {
                    if (run != 15) break;  // end of block
                    k += 16;
                    continue;
                }
                k += run;
                if (k > 63) {
                    reason = GANCE_JPEG_INVALID_CODE;
                    break;
                }
                const int value = extend((int)reader.peek(size), size);
                reader.skip(size);
                const int n = natural[k];
                slot[((n >> 1) * kEntropyThreads + tid) * 2 + (n & 1)] = (int16_t)value;
                ++k;
            }
            if (reason == GANCE_JPEG_OK && reader.overrun()) reason = GANCE_JPEG_TRUNCATED;
            uint4* dst = (uint4*)(coef + (((int64_t)frame * mcus + mcu) * kBlocks + kind) * 64);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                uint32_t* w = slots + 4 * i * kEntropyThreads + tid;
                dst[i] = make_uint4(w[0], w[kEntropyThreads], w[2 * kEntropyThreads], w[3 * kEntropyThreads]);
                w[0] = w[kEntropyThreads] = w[2 * kEntropyThreads] = w[3 * kEntropyThreads] = 0;
            }
        }
    }
    if (reason != GANCE_JPEG_OK) atomicMax(status + frame, reason);
}

// ---- 3. dequantisation and IDCT ------------------------------------------------------------------------------------
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
              FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
              FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jpeg_idct_islow on one column / row: 8 values at stride `step`, descaled by `shift`
template <int shift>
__device__ __forceinline__ void idct_1d(int* d, int step) {
    int z2 = d[2 * step], z3 = d[6 * step];
    int z1 = (z2 + z3) * FIX_0_541196100;
    int tmp2 = z1 + z3 * -FIX_1_847759065;
    int tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = d[0 * step], z3 = d[4 * step];
    int tmp0 = (z2 + z3) * (1 << kConstBits), tmp1 = (z2 - z3) * (1 << kConstBits);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7 * step], tmp1 = d[5 * step], tmp2 = d[3 * step], tmp3 = d[1 * step];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 *= FIX_0_298631336, tmp1 *= FIX_2_053119869, tmp2 *= FIX_3_072711026, tmp3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223, z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5;
    z4 = z4 * -FIX_0_390180644 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    d[0 * step] = descale(tmp10 + tmp3, shift), d[7 * step] = descale(tmp10 - tmp3, shift);
    d[1 * step] = descale(tmp11 + tmp2, shift), d[6 * step] = descale(tmp11 - tmp2, shift);
    d[2 * step] = descale(tmp12 + tmp1, shift), d[5 * step] = descale(tmp12 - tmp1, shift);
    d[3 * step] = descale(tmp13 + tmp0, shift), d[4 * step] = descale(tmp13 - tmp0, shift);
}

// The level shift and saturation of libjpeg-turbo's SIMD islow IDCT (signed saturating packs, then + 128). The C
// fallback's sample_range_limit[value & 0x3FF] gives the same for |value| < 512 and wraps beyond; the decoders PIL
// ships run the SIMD path.
__host__ __device__ __forceinline__ uint32_t range_limit(int value) { return (uint32_t)min(255, max(0, value + 128)); }

// Where the blocks of an MCU go: block k < luma_blocks is the Y block at block row k >> h_shift, column k & h_mask of
// its MCU (h_shift = log2 of the luma's horizontal factor), the two after them are Cb and Cr. Rows per plane and the
// bytes between rows as Layout has them.
struct PlaneMap {
    int blocks_per_mcu, luma_blocks, h_shift, v_blocks;
    int luma_stride, luma_rows, chroma_stride, chroma_rows;
};

// One thread per block, numbered kind-major inside a frame so that a wave works on one component's table and plane.
__global__ void __launch_bounds__(256) mjpeg_idct_kernel(const int16_t* __restrict__ coef, const FrameDesc* __restrict__ frames,
                                                         const TableSet* __restrict__ sets, int mcus, int mcu_cols, int64_t blocks, PlaneMap map,
                                                         uint8_t* __restrict__ luma, uint8_t* __restrict__ chroma_b, uint8_t* __restrict__ chroma_r) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= blocks) return;
    const int64_t frame = t / (map.blocks_per_mcu * (int64_t)mcus);
    const int within = (int)(t - frame * map.blocks_per_mcu * mcus);
    const int kind = within / mcus, mcu = within - kind * mcus;
    const int c = kind < map.luma_blocks ? 0 : kind - map.luma_blocks + 1;
    const uint16_t* quant = sets[frames[frame].table_set].quant[c];
    const uint4* src = (const uint4*)(coef + ((frame * mcus + mcu) * map.blocks_per_mcu + kind) * 64);
    int d[64];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = src[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[8 * i + 2 * j] = (int)(int16_t)(w[j] & 0xFFFF) * quant[8 * i + 2 * j];
            d[8 * i + 2 * j + 1] = (int)(int16_t)(w[j] >> 16) * quant[8 * i + 2 * j + 1];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) idct_1d<kConstBits - kPass1Bits>(d + i, 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) idct_1d<kConstBits + kPass1Bits + 3>(d + 8 * i, 1);
    const int mcu_row = mcu / mcu_cols, mcu_col = mcu - mcu_row * mcu_cols;
    uint8_t* plane;
    int64_t width, x0, row0;
    if (kind < map.luma_blocks) {
        const int block_row = kind >> map.h_shift, block_col = kind - (block_row << map.h_shift);
        plane = luma, width = map.luma_stride;
        x0 = ((mcu_col << map.h_shift) + block_col) * 8;
        row0 = frame * map.luma_rows + (mcu_row * map.v_blocks + block_row) * 8;
    } else {
        plane = kind == map.luma_blocks ? chroma_b : chroma_r, width = map.chroma_stride;
        x0 = mcu_col * 8;
        row0 = frame * map.chroma_rows + mcu_row * 8;
    }
    uint8_t* dst = plane + row0 * width + x0;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        uint2 row;
        row.x = range_limit(d[8 * y]) | range_limit(d[8 * y + 1]) << 8 | range_limit(d[8 * y + 2]) << 16 | range_limit(d[8 * y + 3]) << 24;
        row.y = range_limit(d[8 * y + 4]) | range_limit(d[8 * y + 5]) << 8 | range_limit(d[8 * y + 6]) << 16 | range_limit(d[8 * y + 7]) << 24;
        *(uint2*)(dst + y * width) = row;  // 8-byte aligned: planes start 16-byte aligned, strides are multiples of 8
    }
}

// ---- 4. upsampling and colour --------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(255, max(0, v)); }

// What the colour kernels are told about the planes
struct ColourArgs {
    int width, height, groups_per_row;  // groups of 16 pixels
    int luma_stride, luma_rows, chroma_stride, chroma_rows;
    int64_t groups;  // of the call
    int wide;        // width is a multiple of 16 and d_out is 16-byte aligned: the 48 bytes go out as three 16-byte stores
};

// in[0 .. 9] = samples i0 - 1 .. i0 + 8 of a chroma row (0 where the true width ends)
__device__ __forceinline__ void load_chroma10(const uint8_t* __restrict__ row, int i0, int chroma_width, int* in) {
    const uint2 v = *(const uint2*)(row + i0);
#pragma unroll
    for (int i = 0; i < 4; ++i) in[1 + i] = (v.x >> (8 * i)) & 0xFF, in[5 + i] = (v.y >> (8 * i)) & 0xFF;
    in[0] = i0 > 0 ? row[i0 - 1] : 0;
    in[9] = i0 + 8 < chroma_width ? row[i0 + 8] : 0;
}

// One thread per 16 pixels of an output row; kLayout picks the upsampling (jdsample.c), all of it in integers:
//   4:2:2  h2v1_fancy_upsample: 3/4 of the nearer sample, 1/4 of the further, over the true chroma width
//   4:2:0  h2v2_fancy_upsample: per column 3 * nearer row + further row, then the same triangle along the row; the
//          further row is r - 1 for output row 2r, r + 1 for 2r + 1, clamped to the true plane [0, ceil(H / 2) - 1]: never a
//          padding row of the blocks, and rows of the neighbouring MCU row where there is one
//   both   sample replication (h2v1_upsample / h2v2_upsample) when the true chroma width is at most 2, as libjpeg picks
//   4:4:4  the sample itself; grey: no chroma planes, the three channels are the luma sample
template <int kLayout>
__global__ void __launch_bounds__(256) mjpeg_colour_kernel(const uint8_t* __restrict__ luma, const uint8_t* __restrict__ chroma_b,
                                                           const uint8_t* __restrict__ chroma_r, ColourArgs a, uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.groups) return;
    const int group = (int)(t % a.groups_per_row);
    const int64_t line = t / a.groups_per_row;  // frame * height + y
    const int64_t frame = line / a.height;
    const int y = (int)(line - frame * a.height);
    const int width = a.width;
    const int chroma_width = (width + 1) / 2;  // the component's true width: the upsampler's edges are there
    const uint4 luma16 = *(const uint4*)(luma + (frame * a.luma_rows + y) * (int64_t)a.luma_stride + group * 16);
    const uint32_t lw[4] = {luma16.x, luma16.y, luma16.z, luma16.w};
    uint8_t rgb[48];
    const uint8_t* planes[2] = {chroma_b, chroma_r};
    int up[2][16];
    if constexpr (kLayout == GANCE_JPEG_LAYOUT_422) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i0 = group * 8;
            int in[10];
            load_chroma10(planes[p] + (frame * a.chroma_rows + y) * (int64_t)a.chroma_stride, i0, chroma_width, in);
            if (chroma_width > 2) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int index = i0 + i;
                    up[p][2 * i] = index == 0 ? in[1 + i] : (3 * in[1 + i] + in[i] + 1) >> 2;
                    up[p][2 * i + 1] = index >= chroma_width - 1 ? in[1 + i] : (3 * in[1 + i] + in[2 + i] + 2) >> 2;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) up[p][2 * i] = up[p][2 * i + 1] = in[1 + i];
            }
        }
    } else if constexpr (kLayout == GANCE_JPEG_LAYOUT_420) {
        const int chroma_height = (a.height + 1) / 2;
        const int near_row = y >> 1;  // < chroma_height <= chroma_rows
        const int far_row = (y & 1) ? min(near_row + 1, chroma_height - 1) : max(near_row - 1, 0);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i0 = group * 8;
            const uint8_t* plane = planes[p] + frame * a.chroma_rows * (int64_t)a.chroma_stride;
            int in[10], far[10];
            load_chroma10(plane + near_row * (int64_t)a.chroma_stride, i0, chroma_width, in);
            if (chroma_width > 2) {
                load_chroma10(plane + far_row * (int64_t)a.chroma_stride, i0, chroma_width, far);
#pragma unroll
                for (int i = 0; i < 10; ++i) in[i] = 3 * in[i] + far[i];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int index = i0 + i;
                    up[p][2 * i] = (3 * in[1 + i] + (index == 0 ? in[1 + i] : in[i]) + 8) >> 4;
                    up[p][2 * i + 1] = (3 * in[1 + i] + (index >= chroma_width - 1 ? in[1 + i] : in[2 + i]) + 7) >> 4;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) up[p][2 * i] = up[p][2 * i + 1] = in[1 + i];
            }
        }
    } else if constexpr (kLayout == GANCE_JPEG_LAYOUT_444) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const uint4 v = *(const uint4*)(planes[p] + (frame * a.chroma_rows + y) * (int64_t)a.chroma_stride + group * 16);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int x = 0; x < 16; ++x) up[p][x] = (w[x >> 2] >> (8 * (x & 3))) & 0xFF;
        }
    }
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int luminance = (lw[x >> 2] >> (8 * (x & 3))) & 0xFF;
        if constexpr (kLayout == GANCE_JPEG_LAYOUT_GREY) {
            rgb[3 * x] = rgb[3 * x + 1] = rgb[3 * x + 2] = (uint8_t)luminance;
        } else {
            const int cb = up[0][x] - 128, cr = up[1][x] - 128;
            rgb[3 * x] = (uint8_t)clamp255(luminance + ((91881 * cr + 32768) >> 16));
            rgb[3 * x + 1] = (uint8_t)clamp255(luminance + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
            rgb[3 * x + 2] = (uint8_t)clamp255(luminance + ((116130 * cb + 32768) >> 16));
        }
    }
    uint8_t* dst = out + (line * width + group * 16) * 3;
    if (a.wide) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                w[j] = rgb[16 * i + 4 * j] | rgb[16 * i + 4 * j + 1] << 8 | rgb[16 * i + 4 * j + 2] << 16 | (uint32_t)rgb[16 * i + 4 * j + 3] << 24;
            ((uint4*)dst)[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        const int count = min(16, width - group * 16) * 3;
#pragma unroll
        for (int i = 0; i < 48; ++i)
            if (i < count) dst[i] = rgb[i];
    }
}

// ---- host: tables of a call ----------------------------------------------------------------------------------------
static void derive_table(const uint8_t bits[16], const uint8_t* values, DeviceTable* table) {
    std::memset(table, 0, sizeof(*table));
    std::memcpy(table->values, values, 256);
    int code = 0, k = 0;
    for (int length = 1; length <= 16; ++length) {
        table->valoff[length] = k - code;
        for (int i = 0; i < bits[length - 1]; ++i, ++k, ++code) {
            if (length > kLookBits) continue;
            const int spare = kLookBits - length;
            for (int j = 0; j < (1 << spare); ++j) table->fast[(code << spare) + j] = (uint16_t)(length << 8 | values[k]);
        }
        table->maxcode[length] = bits[length - 1] ? code - 1 : -1;
        code <<= 1;
    }
}

static size_t tables_offset() { return offsetof(gance_jpeg_info, quant); }
static size_t tables_bytes() { return sizeof(gance_jpeg_info) - tables_offset(); }

// The pinned buffer the per-call tables are copied from. One call at a time fills it; the next waits for the previous
// call's copy (not its kernels) through `copied`.
struct Staging {
    std::mutex mutex;
    void* host = nullptr;
    size_t capacity = 0;
    hipEvent_t copied = nullptr;
};
static Staging g_staging;

template <int kLayout>
static void launch_entropy_and_colour(const Layout& l, int32_t batch, int max_segments, const uint8_t* d_data, const FrameDesc* d_frames,
                                      const TableSet* d_sets, const int32_t* marker_pos, const int32_t* scan_end, int32_t* d_status, int16_t* coef,
                                      const PlaneMap& map, int64_t blocks, uint8_t* luma, uint8_t* chroma_b, uint8_t* chroma_r, const ColourArgs& colour,
                                      uint8_t* d_out, hipStream_t stream) {
    constexpr int kBlocks = kLayout == GANCE_JPEG_LAYOUT_420 ? 6 : (kLayout == GANCE_JPEG_LAYOUT_444 ? 3 : (kLayout == GANCE_JPEG_LAYOUT_GREY ? 1 : 4));
    const dim3 entropy_grid((unsigned)((max_segments + kEntropyThreads - 1) / kEntropyThreads), (unsigned)batch);
    mjpeg_entropy_kernel<kBlocks><<<entropy_grid, kEntropyThreads, 0, stream>>>(d_data, d_frames, d_sets, marker_pos, scan_end, d_status, coef, (int)l.mcus);
    mjpeg_idct_kernel<<<(unsigned)((blocks + 255) / 256), 256, 0, stream>>>(coef, d_frames, d_sets, (int)l.mcus, (int)l.mcu_cols, blocks, map, luma, chroma_b,
                                                                           chroma_r);
    mjpeg_colour_kernel<kLayout><<<(unsigned)((colour.groups + 255) / 256), 256, 0, stream>>>(luma, chroma_b, chroma_r, colour, d_out);
}

// The decode of both entries. Frame b's description is at infos + b * info_stride: an array of gance_jpeg_info, or of
// gance_jpeg_frame_info, whose first member it is. `layout` is the one layout of all frames.
static int decode(const uint8_t* d_data, const int64_t* h_offsets, const char* infos, size_t info_stride, int layout, int32_t batch,
                  void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, int32_t* d_status, void* stream_ptr, const char* bounds_name) {
    if (batch < 1) return fail("batch must be >= 1");
    const gance_jpeg_info& first = *(const gance_jpeg_info*)infos;
    const int width = first.width, height = first.height;
    if (width < 1 || width > kMaxSide || height < 1 || height > kMaxSide)
        return fail("width and height must be in [1, " + std::to_string(kMaxSide) + "], got " + std::to_string(width) + " x " + std::to_string(height));
    if ((uintptr_t)d_workspace % 16 != 0) return fail("workspace must be 16-byte aligned");
    if (h_offsets[0] < 0) return fail("offsets must not be negative");
    const Layout l = layout_of(batch, width, height, layout);
    if (l.max_markers > INT32_MAX) return fail("batch of " + std::to_string(batch) + " frames of this size: split the call");

    std::vector<FrameDesc> descs((size_t)batch);
    std::vector<const gance_jpeg_info*> distinct;
    int64_t marker_base = 0;
    int max_segments = 1;
    for (int32_t b = 0; b < batch; ++b) {
        const gance_jpeg_info& info = *(const gance_jpeg_info*)(infos + (size_t)b * info_stride);
        const std::string name = "frame " + std::to_string(b);
        const int64_t file_bytes = h_offsets[b + 1] - h_offsets[b];
        if (file_bytes < 0 || file_bytes > INT32_MAX) return fail(name + ": a file of " + std::to_string(file_bytes) + " bytes");
        if (info.width != width || info.height != height)
            return fail(name + " is " + std::to_string(info.width) + " x " + std::to_string(info.height) + ", frame 0 is " +
                        std::to_string(width) + " x " + std::to_string(height) + ": the frames of one call must have one size");
        if (info.scan_offset > (uint64_t)file_bytes || info.scan_offset + info.scan_bytes != (uint64_t)file_bytes)
            return fail(name + ": the scan range does not end with the file");
        if (info.restart_interval < 0 || info.restart_interval > 65535) return fail(name + ": restart interval " + std::to_string(info.restart_interval));
        for (int c = 0; c < l.shape.components; ++c)
            for (int cls = 0; cls < 2; ++cls) {
                std::string why;
                if (table_error(info.huff_bits[c][cls], info.huff_values[c][cls], cls == 0, &why)) return fail(name + ": " + why);
            }
        int set = -1;
        for (int s = (int)distinct.size() - 1; s >= 0 && set < 0; --s)
            if (std::memcmp((const char*)distinct[s] + tables_offset(), (const char*)&info + tables_offset(), tables_bytes()) == 0) set = s;
        if (set < 0) set = (int)distinct.size(), distinct.push_back(&info);
        FrameDesc& d = descs[b];
        d.scan_begin = h_offsets[b] + (int64_t)info.scan_offset;
        d.scan_bytes = (int32_t)info.scan_bytes;
        d.restart_interval = info.restart_interval;
        d.segments = info.restart_interval > 0 ? (int32_t)((l.mcus + info.restart_interval - 1) / info.restart_interval) : 1;
        d.marker_base = (int32_t)marker_base;
        d.table_set = set;
        d.reserved = 0;
        marker_base += d.segments - 1;
        if (d.segments > max_segments) max_segments = d.segments;
    }
    if (workspace_bytes < (uint64_t)l.workspace_bytes)
        return fail("workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.workspace_bytes) +
                    " needed (" + bounds_name + ")");

    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return gance::set_last_error(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    gance::DeviceGuard guard(gance::device_of_pointer(d_data));  // launch where the bytes live
    if (guard.status() != hipSuccess)
        return gance::set_last_error(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));
    hipStream_t stream = (hipStream_t)stream_ptr;

    const size_t desc_bytes = (size_t)round16(batch * (int64_t)sizeof(FrameDesc));
    const size_t upload_bytes = desc_bytes + distinct.size() * sizeof(TableSet);
    {
        std::lock_guard<std::mutex> lock(g_staging.mutex);
        hipError_t err = hipSuccess;
        if (g_staging.copied != nullptr) {
            err = hipEventSynchronize(g_staging.copied);
            (void)hipEventDestroy(g_staging.copied);
            g_staging.copied = nullptr;
        }
        if (err == hipSuccess && g_staging.capacity < upload_bytes) {
            if (g_staging.host != nullptr) (void)hipHostFree(g_staging.host);
            g_staging.host = nullptr, g_staging.capacity = 0;
            err = hipHostMalloc(&g_staging.host, upload_bytes, hipHostMallocPortable);
            if (err == hipSuccess) g_staging.capacity = upload_bytes;
        }
        if (err == hipSuccess) {
            char* host = (char*)g_staging.host;
            std::memset(host, 0, desc_bytes);
            std::memcpy(host, descs.data(), (size_t)batch * sizeof(FrameDesc));
            TableSet* sets = (TableSet*)(host + desc_bytes);
            for (size_t s = 0; s < distinct.size(); ++s) {
                std::memset((void*)&sets[s], 0, sizeof(TableSet));  // grey: the chroma slots stay zero and are not read
                for (int c = 0; c < l.shape.components; ++c) {
                    derive_table(distinct[s]->huff_bits[c][0], distinct[s]->huff_values[c][0], &sets[s].huff[c][0]);
                    derive_table(distinct[s]->huff_bits[c][1], distinct[s]->huff_values[c][1], &sets[s].huff[c][1]);
                    for (int i = 0; i < 64; ++i) sets[s].quant[c][i] = distinct[s]->quant[c][i];
                }
            }
            err = hipMemcpyAsync(d_workspace, host, upload_bytes, hipMemcpyHostToDevice, stream);
        }
        if (err == hipSuccess) err = hipEventCreateWithFlags(&g_staging.copied, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventRecord(g_staging.copied, stream);
        if (err != hipSuccess) return gance::set_last_error(GANCE_ERR_HIP, std::string("mjpeg decode tables: ") + hipGetErrorString(err));
    }

    char* ws = (char*)d_workspace;
    const FrameDesc* d_frames = (const FrameDesc*)ws;
    const TableSet* d_sets = (const TableSet*)(ws + desc_bytes);
    char* at = ws + l.params_bytes;
    int32_t* marker_pos = (int32_t*)at;
    at += l.marker_bytes;
    int32_t* scan_end = (int32_t*)at;
    at += l.end_bytes;
    int16_t* coef = (int16_t*)at;
    at += l.coef_bytes;
    uint8_t* luma = (uint8_t*)at;
    at += l.luma_bytes;
    uint8_t* chroma_b = (uint8_t*)at;  // grey: no chroma planes, never read
    uint8_t* chroma_r = (uint8_t*)(at + l.chroma_bytes);

    mjpeg_marker_scan_kernel<<<(unsigned)batch, kScanThreads, 0, stream>>>(d_data, d_frames, marker_pos, scan_end, d_status);
    PlaneMap map{};
    map.blocks_per_mcu = l.shape.blocks_per_mcu, map.luma_blocks = l.shape.h * l.shape.v, map.h_shift = l.shape.h - 1, map.v_blocks = l.shape.v;
    map.luma_stride = (int)l.luma_stride, map.luma_rows = (int)l.luma_rows, map.chroma_stride = (int)l.chroma_stride, map.chroma_rows = (int)l.chroma_rows;
    const int64_t blocks = (int64_t)batch * l.mcus * l.shape.blocks_per_mcu;
    ColourArgs colour{};
    colour.width = width, colour.height = height, colour.groups_per_row = (width + 15) / 16;
    colour.luma_stride = map.luma_stride, colour.luma_rows = map.luma_rows, colour.chroma_stride = map.chroma_stride, colour.chroma_rows = map.chroma_rows;
    colour.groups = (int64_t)batch * height * colour.groups_per_row;
    colour.wide = width % 16 == 0 && (uintptr_t)d_out % 16 == 0;
#define GANCE_LAUNCH(kLayout)                                                                                                                        \
    launch_entropy_and_colour<kLayout>(l, batch, max_segments, d_data, d_frames, d_sets, marker_pos, scan_end, d_status, coef, map, blocks, luma, \
                                       chroma_b, chroma_r, colour, d_out, stream)
    switch (layout) {
        case GANCE_JPEG_LAYOUT_420: GANCE_LAUNCH(GANCE_JPEG_LAYOUT_420); break;
        case GANCE_JPEG_LAYOUT_444: GANCE_LAUNCH(GANCE_JPEG_LAYOUT_444); break;
        case GANCE_JPEG_LAYOUT_GREY: GANCE_LAUNCH(GANCE_JPEG_LAYOUT_GREY); break;
        default: GANCE_LAUNCH(GANCE_JPEG_LAYOUT_422); break;
    }
#undef GANCE_LAUNCH
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return gance::set_last_error(GANCE_ERR_HIP, std::string("mjpeg decode launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

}  // namespace gance_mjpeg_decode

extern "C" {

static int bounds(const char* entry, int32_t batch, int32_t width, int32_t height, int32_t layout, uint64_t* workspace_bytes) {
    using namespace gance_mjpeg_decode;
    if (workspace_bytes == nullptr) return fail(std::string("NULL argument to ") + entry);
    if (batch < 1) return fail("batch must be >= 1");
    if (width < 1 || width > kMaxSide || height < 1 || height > kMaxSide)
        return fail("width and height must be in [1, " + std::to_string(kMaxSide) + "], got " + std::to_string(width) + " x " + std::to_string(height));
    *workspace_bytes = (uint64_t)layout_of(batch, width, height, layout).workspace_bytes;
    return GANCE_OK;
}

// (the workspace is sized by the geometry alone; total_bytes is part of the queries so that it may depend on it)
int gance_jpeg_decode_bounds(int32_t batch, int32_t width, int32_t height, uint64_t total_bytes, uint64_t* workspace_bytes) {
    (void)total_bytes;
    return bounds("gance_jpeg_decode_bounds", batch, width, height, GANCE_JPEG_LAYOUT_422, workspace_bytes);
}

int gance_jpeg_decode_layouts_bounds(int32_t batch, int32_t width, int32_t height, int32_t layout, uint64_t total_bytes, uint64_t* workspace_bytes) {
    using namespace gance_mjpeg_decode;
    (void)total_bytes;
    if (layout < GANCE_JPEG_LAYOUT_422 || layout > GANCE_JPEG_LAYOUT_GREY) return fail("layout must be one of GANCE_JPEG_LAYOUT_*, got " + std::to_string(layout));
    return bounds("gance_jpeg_decode_layouts_bounds", batch, width, height, layout, workspace_bytes);
}

int gance_jpeg_decode_u8(const uint8_t* d_data, const int64_t* h_offsets, const gance_jpeg_info* infos, int32_t batch, void* d_workspace,
                         uint64_t workspace_bytes, uint8_t* d_out, int32_t* d_status, void* stream) {
    using namespace gance_mjpeg_decode;
    if (d_data == nullptr || h_offsets == nullptr || infos == nullptr || d_workspace == nullptr || d_out == nullptr || d_status == nullptr)
        return fail("NULL argument to gance_jpeg_decode_u8");
    return decode(d_data, h_offsets, (const char*)infos, sizeof(gance_jpeg_info), GANCE_JPEG_LAYOUT_422, batch, d_workspace, workspace_bytes, d_out,
                  d_status, stream, "gance_jpeg_decode_bounds");
}

int gance_jpeg_decode_layouts_u8(const uint8_t* d_data, const int64_t* h_offsets, const gance_jpeg_frame_info* infos, int32_t batch,
                                 void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, int32_t* d_status, void* stream) {
    using namespace gance_mjpeg_decode;
    if (d_data == nullptr || h_offsets == nullptr || infos == nullptr || d_workspace == nullptr || d_out == nullptr || d_status == nullptr)
        return fail("NULL argument to gance_jpeg_decode_layouts_u8");
    if (batch < 1) return fail("batch must be >= 1");
    const int layout = infos[0].layout;
    if (layout < GANCE_JPEG_LAYOUT_422 || layout > GANCE_JPEG_LAYOUT_GREY) return fail("frame 0: layout " + std::to_string(layout));
    static const char* const names[4] = {"4:2:2", "4:2:0", "4:4:4", "grey"};
    for (int32_t b = 1; b < batch; ++b)
        if (infos[b].layout != layout)
            return fail("frame " + std::to_string(b) + " is " + (infos[b].layout >= 0 && infos[b].layout <= 3 ? names[infos[b].layout] : "of an unknown layout") +
                        ", frame 0 is " + names[layout] + ": the frames of one call must have one layout");
    return decode(d_data, h_offsets, (const char*)infos, sizeof(gance_jpeg_frame_info), layout, batch, d_workspace, workspace_bytes, d_out, d_status,
                  stream, "gance_jpeg_decode_layouts_bounds");
}

}  // extern "C"
