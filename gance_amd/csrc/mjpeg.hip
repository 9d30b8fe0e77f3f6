// Baseline JPEG (JFIF, 4:2:2, standard Huffman tables, one restart interval per MCU row) of uint8 frames in HBM:
// gance_jpeg_encode_bounds / gance_jpeg_encode_u8 (square frames) and gance_jpeg_encode_rect_bounds /
// gance_jpeg_encode_rect_u8 (width x height, the square entries call them) of include/gance_hip.h. The arithmetic is libjpeg's "islow" path, so
// libjpeg decodes our files to exactly the pixels it decodes from its own encode at the same quality:
//
//   RGB -> YCbCr        jccolor.c rgb_ycc_convert: 16-bit fixed point, Y rounded half up, Cb/Cr with ONE_HALF - 1
//   4:2:2 downsampling  jcsample.c h2v1_downsample: (a + b + bias) >> 1, bias 0 / 1 on even / odd output columns
//   forward DCT         jfdctint.c jpeg_fdct_islow: Loeffler-Ligtenberg-Moschytz, CONST_BITS 13, PASS1_BITS 2
//   quantisation        jcdctmgr.c: sign(c) * ((|c| + d/2) / d) with d = 8 q, exact (multiply-high by ceil(2^32 / d))
//   quality scaling     jcparam.c jpeg_quality_scaling + jpeg_add_quant_table (force_baseline)
//   Huffman coding      jchuff.c encode_one_block with the Annex K tables, restart markers as emit_restart
//
// Four launches, all on the caller's stream, deterministic (no atomics, no order-dependent reduction):
//   1. mjpeg_transform_kernel  one thread per 8x8 block: colour, downsampling, DCT, quantisation -> int16 zigzag
//   2. mjpeg_huffman_kernel    one thread per block: its Huffman bits (DC as a difference to the previous block of the
//                              same component inside the MCU row) into a private 52-word slot + the bit count
//   3. mjpeg_segment_kernel    one workgroup per restart segment (one MCU row of one frame): scan of the bit counts,
//                              every output word gathered from the blocks that overlap it, 1-padding, 0xFF 0x00
//                              stuffing by a second scan, bytes into the segment's slot
//   4. mjpeg_frame_layout_kernel, mjpeg_frame_offsets_kernel, mjpeg_pack_kernel   block scans of the segment sizes
//                              per frame and of the frame sizes, then header + segments + RSTn + EOI per frame, frames
//                              back to back
// Every buffer is sized for the worst case (a block is at most 1660 bits before stuffing), so nothing can truncate.
//
// The optimised mode (gance_jpeg_encode_rect_optimized_*, libjpeg's optimize_coding) codes each frame with the optimal
// tables of its own symbols. Between launches 1 and 3 it runs, in place of launch 2:
//   2a. mjpeg_symbol_count_kernel    one thread per block, the walk of launch 2 with + 1 on a symbol in place of its bits:
//                                    histograms in LDS, flushed into per-frame counts (integer atomics: order-independent)
//   2b. mjpeg_optimal_tables_kernel  one wave per (frame, table): jchuff.c jpeg_gen_optimal_table, then the frame's DHT
//                                    segments and encoder views (gance_jpeg_optimal_tables is this kernel on given counts)
//   2c. mjpeg_huffman_frame_kernel   launch 2 with the frame's tables staged in LDS
// and the layout and pack kernels take a header length per frame. The standard mode's kernels are the code they were.

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"
#include "mjpeg_tables.h"

namespace gance_mjpeg {

constexpr int kMaxSide = 8192;            // segments of up to 2048 blocks: their bit offsets fit the segment kernel's LDS
constexpr int kMaxBlockBits = 1660;       // 16 + 11 (DC) + 63 x (16 + 10) (AC)
constexpr int kBlockWords = 52;           // ceil(1660 / 32)
constexpr int kSegmentThreads = 256;
constexpr int kMaxSegmentBlocks = 4 * (kMaxSide / 16);
constexpr int kHeaderCapacity = 640;

// Encoder view of a table (jchuff.c jpeg_make_c_derived_tbl): code and length per symbol (length 0 = unused)
struct HuffTable {
    uint16_t code[256];
    uint8_t size[256];
};
struct HuffTables {
    HuffTable dc[2], ac[2];  // [0] luma, [1] chroma
};

constexpr HuffTable derive(const uint8_t* bits, const uint8_t* values) {
    HuffTable table{};
    int code = 0, k = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int i = 0; i < bits[length - 1]; ++i, ++k) {
            table.code[values[k]] = (uint16_t)code++;
            table.size[values[k]] = (uint8_t)length;
        }
        code <<= 1;
    }
    return table;
}

constexpr HuffTables make_tables() {
    return HuffTables{{derive(kDcLumaBits, kDcValues), derive(kDcChromaBits, kDcValues)},
                      {derive(kAcLumaBits, kAcLumaValues), derive(kAcChromaBits, kAcChromaValues)}};
}

__constant__ HuffTables kHuff = make_tables();

// The four tables in the order of a file's DHT segments: DC luma, AC luma, DC chroma, AC chroma. A frame of the optimised
// mode carries its own four: the DHT payloads (class byte, 16 counts, symbols) and the encoder views in this order.
constexpr int kFrameTables = 4;
constexpr int kDhtCapacity = 4 * (2 + 2 + 1 + 16) + 2 * (12 + 162);  // 432: what the Annex K tables take as well

struct StandardDht {
    uint8_t bits[kFrameTables][16];
    uint8_t values[kFrameTables][162];
};

constexpr StandardDht make_standard_dht() {
    StandardDht d{};
    const uint8_t* bits[kFrameTables] = {kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits};
    const uint8_t* values[kFrameTables] = {kDcValues, kAcLumaValues, kDcValues, kAcChromaValues};
    for (int t = 0; t < kFrameTables; ++t) {
        int count = 0;
        for (int i = 0; i < 16; ++i) d.bits[t][i] = bits[t][i], count += bits[t][i];
        for (int i = 0; i < count; ++i) d.values[t][i] = values[t][i];
    }
    return d;
}

__constant__ StandardDht kStandardDht = make_standard_dht();

// Quantisation of one quality, natural order: d / 2 and ceil(2^32 / d) with d = 8 q (the islow DCT's output is 8x)
struct QuantArgs {
    uint32_t half[2][64];
    uint32_t magic[2][64];
};

// Table entries at `quality` (jpeg_set_quality with force_baseline), natural order
static void scaled_table(int component, int quality, int out[64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int i = 0; i < 64; ++i) {
        long v = ((long)kBaseQuant[component][i] * scale + 50) / 100;
        out[i] = (int)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

static QuantArgs make_quant(int quality) {
    QuantArgs args{};
    for (int c = 0; c < 2; ++c) {
        int table[64];
        scaled_table(c, quality, table);
        for (int i = 0; i < 64; ++i) {
            const uint64_t d = 8ull * table[i];
            args.half[c][i] = (uint32_t)(d / 2);
            // exact for every dividend below 2^16 (|c| + d/2 < 2^15 here): ceil(2^32/d) d - 2^32 < d <= 2^16
            args.magic[c][i] = (uint32_t)(((1ull << 32) + d - 1) / d);
        }
    }
    return args;
}

struct Header {
    uint8_t bytes[kHeaderCapacity];
    int length;
    int dht_begin, dht_end;  // the four DHT segments are bytes [dht_begin, dht_end)
};

// SOI, APP0 (JFIF 1.01, aspect 1:1), DQT x2 (zigzag), SOF0 (Y 2x1, Cb 1x1, Cr 1x1), DHT x4, DRI, SOS
static Header make_header(int width, int height, int quality) {
    Header h{};
    int n = 0;
    auto put = [&](int v) { h.bytes[n++] = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 0xFF); };
    put16(0xFFD8);
    put16(0xFFE0); put16(16);
    for (char c : {'J', 'F', 'I', 'F', '\0'}) put(c);
    put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
    for (int c = 0; c < 2; ++c) {
        int table[64];
        scaled_table(c, quality, table);
        put16(0xFFDB); put16(67); put(c);
        for (int i = 0; i < 64; ++i) put(table[natural_of_zigzag(i)]);
    }
    put16(0xFFC0); put16(17); put(8); put16(height); put16(width); put(3);
    put(1); put(0x21); put(0);
    put(2); put(0x11); put(1);
    put(3); put(0x11); put(1);
    const uint8_t* bits[4] = {kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits};
    const uint8_t* values[4] = {kDcValues, kAcLumaValues, kDcValues, kAcChromaValues};
    const int classes[4] = {0x00, 0x10, 0x01, 0x11};
    h.dht_begin = n;
    for (int t = 0; t < 4; ++t) {
        int count = 0;
        for (int i = 0; i < 16; ++i) count += bits[t][i];
        put16(0xFFC4); put16(2 + 1 + 16 + count); put(classes[t]);
        for (int i = 0; i < 16; ++i) put(bits[t][i]);
        for (int i = 0; i < count; ++i) put(values[t][i]);
    }
    h.dht_end = n;
    put16(0xFFDD); put16(4); put16(width / 16);
    put16(0xFFDA); put16(12); put(3);
    put(1); put(0x00);
    put(2); put(0x11);
    put(3); put(0x11);
    put(0); put(63); put(0);
    h.length = n;
    return h;
}

// ---- sizes -------------------------------------------------------------------------------------------------------
struct Layout {
    int64_t mcu_cols, mcu_rows, segment_blocks, segments, blocks;
    int64_t segment_capacity;                       // stuffed bytes of a worst-case segment, rounded to 16
    int64_t coef_bytes, bits_bytes, bitlen_bytes, slot_bytes, size_bytes, dst_bytes;
    int64_t workspace_bytes, frame_capacity, out_capacity;
    // the optimised mode's own regions, after the others (all 0 in the standard mode)
    int64_t count_bytes, table_bytes, dht_bytes, dht_length_bytes, table_bits_bytes, table_values_bytes, table_status_bytes;
};

static int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

static Layout layout_of(int64_t batch, int64_t width, int64_t height, bool optimized = false) {
    Layout l{};
    l.mcu_cols = width / 16;
    l.mcu_rows = height / 8;
    l.segment_blocks = 4 * l.mcu_cols;  // Y0 Y1 Cb Cr per MCU
    l.segments = batch * l.mcu_rows;
    l.blocks = l.segments * l.segment_blocks;
    l.segment_capacity = round16(2 * ((l.segment_blocks * kMaxBlockBits + 7) / 8));  // every byte 0xFF, each stuffed
    l.coef_bytes = round16(l.blocks * 64 * 2);
    l.bits_bytes = round16(l.blocks * kBlockWords * 4);
    l.bitlen_bytes = round16(l.blocks * 4);
    l.slot_bytes = l.segments * l.segment_capacity;
    l.size_bytes = round16(l.segments * 4);
    l.dst_bytes = round16(l.segments * 4);
    l.workspace_bytes = l.coef_bytes + l.bits_bytes + l.bitlen_bytes + l.slot_bytes + l.size_bytes + l.dst_bytes;
    if (optimized) {
        l.count_bytes = batch * kFrameTables * 256 * 4;
        l.table_bytes = batch * kFrameTables * (int64_t)sizeof(HuffTable);
        l.dht_bytes = batch * kDhtCapacity;
        l.dht_length_bytes = round16(batch * 4);
        l.table_bits_bytes = batch * kFrameTables * 16;
        l.table_values_bytes = batch * kFrameTables * 256;
        l.table_status_bytes = batch * kFrameTables * 4;
        l.workspace_bytes += l.count_bytes + l.table_bytes + l.dht_bytes + l.dht_length_bytes + l.table_bits_bytes +
                             l.table_values_bytes + l.table_status_bytes;
    }
    // header + segments + (rows - 1) RST markers + EOI; a frame's own tables take at most the Annex K tables' room in the
    // header (12 and 162 symbols), and a code is at most 16 bits in either mode, so both modes share the capacity
    l.frame_capacity = kHeaderCapacity + l.mcu_rows * (2 * ((l.segment_blocks * kMaxBlockBits + 7) / 8)) + 2 * l.mcu_rows;
    l.out_capacity = batch * l.frame_capacity;
    return l;
}

// ---- 1. transform ------------------------------------------------------------------------------------------------
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
              FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
              FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__host__ __device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jpeg_fdct_islow on one row / column: 8 values at stride `step`; `pass` 0 = rows, 1 = columns
template <int pass>
__host__ __device__ __forceinline__ void fdct_1d(int* d, int step) {
    const int tmp0 = d[0 * step] + d[7 * step], tmp7 = d[0 * step] - d[7 * step];
    const int tmp1 = d[1 * step] + d[6 * step], tmp6 = d[1 * step] - d[6 * step];
    const int tmp2 = d[2 * step] + d[5 * step], tmp5 = d[2 * step] - d[5 * step];
    const int tmp3 = d[3 * step] + d[4 * step], tmp4 = d[3 * step] - d[4 * step];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int odd_shift = pass == 0 ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
    if (pass == 0) {
        d[0 * step] = (tmp10 + tmp11) * (1 << kPass1Bits);
        d[4 * step] = (tmp10 - tmp11) * (1 << kPass1Bits);
    } else {
        d[0 * step] = descale(tmp10 + tmp11, kPass1Bits);
        d[4 * step] = descale(tmp10 - tmp11, kPass1Bits);
    }
    int z1 = (tmp12 + tmp13) * FIX_0_541196100;
    d[2 * step] = descale(z1 + tmp13 * FIX_0_765366865, odd_shift);
    d[6 * step] = descale(z1 - tmp12 * FIX_1_847759065, odd_shift);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    const int t4 = tmp4 * FIX_0_298631336, t5 = tmp5 * FIX_2_053119869, t6 = tmp6 * FIX_3_072711026,
              t7 = tmp7 * FIX_1_501321110;
    z1 *= -FIX_0_899976223;
    z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5;
    z4 = z4 * -FIX_0_390180644 + z5;
    d[7 * step] = descale(t4 + z1 + z3, odd_shift);
    d[5 * step] = descale(t5 + z2 + z4, odd_shift);
    d[3 * step] = descale(t6 + z2 + z3, odd_shift);
    d[1 * step] = descale(t7 + z1 + z4, odd_shift);
}

__host__ __device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
// Cb (cr = false) or Cr of one pixel
__host__ __device__ __forceinline__ int chroma(int r, int g, int b, bool cr) {
    const int v = cr ? 32768 * r - 27439 * g - 5329 * b : -11059 * r - 21709 * g + 32768 * b;
    return (v + (128 << 16) + 32767) >> 16;
}

// Block `kind` (0 / 1 = left / right Y, 2 = Cb, 3 = Cr) of the MCU at (mcu_row, mcu_col) of `frame` [rows][side][3]:
// level-shifted samples, DCT, quantisation; out[64] in zigzag order. `frame` rows are 16-byte aligned (side % 16 == 0).
__host__ __device__ inline void transform_block(const uint8_t* __restrict__ frame, int side, int mcu_row, int mcu_col, int kind,
                                                const QuantArgs& quant, int16_t* __restrict__ out) {
    int d[64];
    const int y0 = mcu_row * 8;
    if (kind < 2) {
        const int x0 = mcu_col * 16 + kind * 8;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint2* row = (const uint2*)(frame + ((size_t)(y0 + y) * side + x0) * 3);  // 24 bytes, 8-byte aligned
            uint8_t px[24];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint2 v = row[i];
                for (int j = 0; j < 4; ++j) px[i * 8 + j] = (uint8_t)(v.x >> (8 * j)), px[i * 8 + 4 + j] = (uint8_t)(v.y >> (8 * j));
            }
#pragma unroll
            for (int x = 0; x < 8; ++x) d[y * 8 + x] = luma(px[3 * x], px[3 * x + 1], px[3 * x + 2]) - 128;
        }
    } else {
        const int x0 = mcu_col * 16;
        const bool cr = kind == 3;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint4* row = (const uint4*)(frame + ((size_t)(y0 + y) * side + x0) * 3);  // 48 bytes, 16-byte aligned
            uint8_t px[48];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint4 v = row[i];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                for (int k = 0; k < 4; ++k)
                    for (int j = 0; j < 4; ++j) px[i * 16 + k * 4 + j] = (uint8_t)(w[k] >> (8 * j));
            }
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int a = chroma(px[6 * x], px[6 * x + 1], px[6 * x + 2], cr);
                const int b = chroma(px[6 * x + 3], px[6 * x + 4], px[6 * x + 5], cr);
                d[y * 8 + x] = ((a + b + (x & 1)) >> 1) - 128;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) fdct_1d<0>(d + 8 * i, 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) fdct_1d<1>(d + i, 8);
    const int c = kind < 2 ? 0 : 1;
#pragma unroll
    for (int z = 0; z < 64; ++z) {
        const int n = natural_of_zigzag(z);
        const int v = d[n];
        const uint32_t a = (uint32_t)(v < 0 ? -v : v) + quant.half[c][n];
        const int q = (int)(((uint64_t)a * quant.magic[c][n]) >> 32);
        out[z] = (int16_t)(v < 0 ? -q : q);
    }
}

// Block index g (within the whole call) <-> (segment, position in the segment). Blocks of a segment are in MCU order:
// MCU m holds positions 4m (Y left), 4m + 1 (Y right), 4m + 2 (Cb), 4m + 3 (Cr). Threads are numbered kind-major
// inside a segment so that a wave works on one kind of block (one code path, adjacent pixels).
__global__ void __launch_bounds__(256) mjpeg_transform_kernel(const uint8_t* __restrict__ frames, int width, int height, int64_t mcu_rows,
                                                              int64_t mcu_cols, int64_t blocks, QuantArgs quant,
                                                              int16_t* __restrict__ coef) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= blocks) return;
    const int64_t segment_blocks = 4 * mcu_cols;
    const int64_t segment = t / segment_blocks;
    const int within = (int)(t - segment * segment_blocks);
    const int kind = within / (int)mcu_cols, mcu = within % (int)mcu_cols;
    const int64_t frame = segment / mcu_rows;
    const int row = (int)(segment - frame * mcu_rows);
    int16_t out[64];
    transform_block(frames + frame * width * height * 3, width, row, mcu, kind, quant, out);
    uint4* dst = (uint4*)(coef + (segment * segment_blocks + 4 * mcu + kind) * 64);
    const uint4* src = (const uint4*)out;
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = src[i];
}

// ---- 2. Huffman bits of one block ----------------------------------------------------------------------------------
struct BitWriter {
    uint64_t acc = 0;
    int pending = 0, total = 0, word = 0;
    uint32_t* out;
    __host__ __device__ explicit BitWriter(uint32_t* o) : out(o) {}
    __host__ __device__ __forceinline__ void put(uint32_t bits, int size) {  // size <= 16
        acc = (acc << size) | (bits & ((1u << size) - 1));
        pending += size;
        total += size;
        if (pending >= 32) {
            pending -= 32;
            out[word++] = (uint32_t)(acc >> pending);
        }
    }
    __host__ __device__ __forceinline__ void finish() {
        if (pending > 0) out[word++] = (uint32_t)(acc << (32 - pending));
    }
};

__host__ __device__ __forceinline__ int bit_length(uint32_t v) { return v == 0 ? 0 : 32 - __builtin_clz(v); }

// jchuff.c encode_one_block on a zigzag-ordered block. The AC loop walks the nonzero coefficients through a bit mask
// (a loop over a runtime index of a local array would put the block in scratch); their values are re-read from
// `block`, which is cached. `words` receives the bits MSB first; returns the bit count (<= kMaxBlockBits).
__host__ __device__ inline int huffman_block(const int16_t* __restrict__ block, int previous_dc, const HuffTable& dc,
                                             const HuffTable& ac, uint32_t* __restrict__ words) {
    uint64_t nonzero = 0;
    int dc_value = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = ((const uint4*)block)[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i == 0 && j == 0) dc_value = (int16_t)(w[0] & 0xFFFF);
            nonzero |= (uint64_t)((w[j] & 0xFFFF) != 0) << (8 * i + 2 * j);
            nonzero |= (uint64_t)((w[j] >> 16) != 0) << (8 * i + 2 * j + 1);
        }
    }
    nonzero &= ~1ull;  // AC only
    BitWriter w(words);
    int temp = dc_value - previous_dc, temp2 = temp;
    if (temp < 0) temp = -temp, --temp2;
    int nbits = bit_length((uint32_t)temp);
    w.put(dc.code[nbits], dc.size[nbits]);
    if (nbits) w.put((uint32_t)temp2, nbits);
    int last = 0;
    while (nonzero) {
        const int k = __builtin_ctzll(nonzero);
        nonzero &= nonzero - 1;
        int run = k - last - 1;
        last = k;
        while (run > 15) {
            w.put(ac.code[0xF0], ac.size[0xF0]);
            run -= 16;
        }
        temp = block[k];
        temp2 = temp;
        if (temp < 0) temp = -temp, --temp2;
        nbits = bit_length((uint32_t)temp);
        const int symbol = (run << 4) + nbits;
        w.put(ac.code[symbol], ac.size[symbol]);
        w.put((uint32_t)temp2, nbits);
    }
    if (last < 63) w.put(ac.code[0], ac.size[0]);
    w.finish();
    return w.total;
}

// Position `p` in a segment -> the position of the previous block of the same component (-1: the segment's first)
__host__ __device__ __forceinline__ int previous_of(int p) {
    const int mcu = p >> 2, kind = p & 3;
    if (kind == 1) return p - 1;
    if (mcu == 0) return -1;
    return kind == 0 ? p - 3 : p - 4;
}

__global__ void __launch_bounds__(256) mjpeg_huffman_kernel(const int16_t* __restrict__ coef, int64_t mcu_cols, int64_t blocks,
                                                            uint32_t* __restrict__ bits, int* __restrict__ bit_counts) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= blocks) return;
    const int64_t segment_blocks = 4 * mcu_cols;
    const int64_t segment = t / segment_blocks;
    const int within = (int)(t - segment * segment_blocks);
    const int kind = within / (int)mcu_cols, mcu = within % (int)mcu_cols;
    const int p = 4 * mcu + kind;
    const int64_t g = segment * segment_blocks + p;
    const int previous = previous_of(p);
    const int previous_dc = previous < 0 ? 0 : coef[(segment * segment_blocks + previous) * 64];
    const int c = kind < 2 ? 0 : 1;
    bit_counts[g] = huffman_block(coef + g * 64, previous_dc, kHuff.dc[c], kHuff.ac[c], bits + g * kBlockWords);
}

// ---- 2b. the optimised mode: a frame's own tables (jchuff.c htest_one_block, jpeg_gen_optimal_table) ------------------
// Thread t of a frame (kind-major inside a segment, as above) -> its block's index in the call and the previous DC
struct FrameBlock {
    int64_t g;
    int previous_dc, component;
};

__device__ __forceinline__ FrameBlock frame_block(const int16_t* __restrict__ coef, int64_t frame, int64_t t, int64_t mcu_cols,
                                                  int64_t frame_blocks) {
    const int64_t segment_blocks = 4 * mcu_cols;
    const int64_t segment = frame * (frame_blocks / segment_blocks) + t / segment_blocks;
    const int within = (int)(t % segment_blocks);
    const int kind = within / (int)mcu_cols, mcu = within % (int)mcu_cols;
    const int p = 4 * mcu + kind;
    const int previous = previous_of(p);
    FrameBlock b;
    b.g = segment * segment_blocks + p;
    b.previous_dc = previous < 0 ? 0 : coef[(segment * segment_blocks + previous) * 64];
    b.component = kind < 2 ? 0 : 1;
    return b;
}

// The symbols huffman_block codes, counted: the walk is the same (the mask of the nonzero coefficients restated, so that
// huffman_block stays the code it was), a put of a code becomes + 1 on its symbol
__device__ inline void count_block(const int16_t* __restrict__ block, int previous_dc, int* __restrict__ dc, int* __restrict__ ac) {
    uint64_t nonzero = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = ((const uint4*)block)[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            nonzero |= (uint64_t)((w[j] & 0xFFFF) != 0) << (8 * i + 2 * j);
            nonzero |= (uint64_t)((w[j] >> 16) != 0) << (8 * i + 2 * j + 1);
        }
    }
    nonzero &= ~1ull;  // AC only
    const int dc_value = block[0];
    int temp = dc_value - previous_dc;
    if (temp < 0) temp = -temp;
    atomicAdd(&dc[bit_length((uint32_t)temp)], 1);
    int last = 0;
    while (nonzero) {
        const int k = __builtin_ctzll(nonzero);
        nonzero &= nonzero - 1;
        int run = k - last - 1;
        last = k;
        if (run > 15) atomicAdd(&ac[0xF0], run >> 4);
        temp = block[k];
        if (temp < 0) temp = -temp;
        atomicAdd(&ac[((run & 15) << 4) + bit_length((uint32_t)temp)], 1);
    }
    if (last < 63) atomicAdd(&ac[0], 1);
}

// counts [frames][4][256], zeroed by the caller: one thread per block, a workgroup's blocks all of one frame. The
// histograms are summed in LDS and then into HBM with integer atomics, so the counts do not depend on the order.
__global__ void __launch_bounds__(256) mjpeg_symbol_count_kernel(const int16_t* __restrict__ coef, int64_t mcu_cols, int64_t frame_blocks,
                                                                 int groups_per_frame, int* __restrict__ counts) {
    __shared__ int histogram[kFrameTables * 256];
    const int64_t frame = blockIdx.x / groups_per_frame;
    const int64_t t = (int64_t)(blockIdx.x % groups_per_frame) * blockDim.x + threadIdx.x;
    for (int i = threadIdx.x; i < kFrameTables * 256; i += blockDim.x) histogram[i] = 0;
    __syncthreads();
    if (t < frame_blocks) {
        const FrameBlock b = frame_block(coef, frame, t, mcu_cols, frame_blocks);
        count_block(coef + b.g * 64, b.previous_dc, histogram + 512 * b.component, histogram + 512 * b.component + 256);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kFrameTables * 256; i += blockDim.x)
        if (histogram[i] != 0) atomicAdd(&counts[frame * kFrameTables * 256 + i], histogram[i]);
}

// The two smallest keys of a wave: (a, b) of every lane merged with the pair of lane ^ d, six times
__device__ __forceinline__ uint64_t shuffle_xor64(uint64_t v, int d) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void wave_two_smallest(uint64_t* a, uint64_t* b) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t oa = shuffle_xor64(*a, d), ob = shuffle_xor64(*b, d);
        const uint64_t low = *a < oa ? *a : oa, high = *a < oa ? oa : *a, rest = *b < ob ? *b : ob;
        *a = low;
        *b = high < rest ? high : rest;
    }
}

constexpr int kTableThreads = 64 * kFrameTables;  // one wave per table, a frame's four in one workgroup

// jpeg_gen_optimal_table of `tables` count vectors [256] (negative counts as 0), one wave each: bits [16], values [256]
// (unused entries 0) and status per table: 0 a table, 1 a code past 32 bits before the limiting (libjpeg's
// JERR_HUFF_CLEN_OVERFLOW), 2 nothing counted; bits and values are 0 unless the status is 0.
// The merge: entry i of the 257 (256 = the reserved symbol, count 1) is held by lane i % 64 with its count, the entry
// that heads its group and its code size. A step takes the two smallest nonzero counts, ties to the larger index (the
// key is count << 9 | 256 - index, smallest first), adds the second into the first and zeroes it, and every lane adds 1
// to the code size of its entries of either group and moves them into the first: what libjpeg's chain walks do.
// With frame_tables (the encoder; tables = 4 per frame in DHT order, a workgroup = a frame) it also writes the frame's
// encoder views, its four DHT segments and their length: the Annex K ones, all four, unless all four statuses are 0 and
// the symbols fit a baseline table (12 DC categories, 162 run/size pairs).
__global__ void __launch_bounds__(kTableThreads) mjpeg_optimal_tables_kernel(const int* __restrict__ counts, int64_t tables,
                                                                             uint8_t* __restrict__ out_bits, uint8_t* __restrict__ out_values,
                                                                             int* __restrict__ out_status, HuffTable* __restrict__ frame_tables,
                                                                             uint8_t* __restrict__ frame_dht, int* __restrict__ frame_dht_length) {
    __shared__ int s_bits[kFrameTables][34];       // symbols per code size, the reserved one included; [33] collects overflows
    __shared__ int s_before[kFrameTables][34];     // symbols 0..255 with a smaller code size (before the limiting)
    __shared__ uint8_t s_size[kFrameTables][256];  // code size per symbol before the limiting
    __shared__ uint8_t s_values[kFrameTables][256];
    __shared__ int s_first_code[kFrameTables][17], s_first_rank[kFrameTables][18];
    __shared__ int s_status[kFrameTables], s_count[kFrameTables];
    __shared__ HuffTable s_table[kFrameTables];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t table = (int64_t)blockIdx.x * kFrameTables + wave;
    const bool active = table < tables;

    int64_t freq[5];
    int group[5], size[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int index = lane + 64 * k;
        int count = 0;
        if (index < 256 && active) count = counts[table * 256 + index];
        if (index == 256) count = 1;
        freq[k] = count > 0 ? count : 0;
        group[k] = index;
        size[k] = 0;
    }
    for (;;) {
        uint64_t a = ~0ull, b = ~0ull;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int index = lane + 64 * k;
            if (index <= 256 && freq[k] > 0) {
                const uint64_t key = ((uint64_t)freq[k] << 9) | (uint64_t)(256 - index);
                if (key < a) b = a, a = key;
                else if (key < b) b = key;
            }
        }
        wave_two_smallest(&a, &b);
        if (b == ~0ull) break;  // one group left
        const int c1 = 256 - (int)(a & 511), c2 = 256 - (int)(b & 511);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int index = lane + 64 * k;
            if (index == c1) freq[k] += (int64_t)(b >> 9);
            if (index == c2) freq[k] = 0;
            if (group[k] == c1 || group[k] == c2) ++size[k], group[k] = c1;
        }
    }

    for (int i = lane; i < 34; i += 64) s_bits[wave][i] = 0, s_before[wave][i] = 0;
    for (int i = lane; i < 256; i += 64) s_table[wave].code[i] = 0, s_table[wave].size[i] = 0, s_values[wave][i] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int index = lane + 64 * k;
        if (index > 256) continue;
        const int clamped = size[k] > 32 ? 33 : size[k];
        if (index < 256) s_size[wave][index] = (uint8_t)clamped;
        if (clamped > 0) atomicAdd(&s_bits[wave][clamped], 1);
        if (clamped > 0 && index < 256) atomicAdd(&s_before[wave][clamped], 1);
    }
    __syncthreads();
    if (lane == 0) {
        int* bits = s_bits[wave];
        int status = 0, total = 0;
        for (int l = 1; l <= 33; ++l) {  // the histogram of the symbols 0..255 into its exclusive prefix
            const int here = s_before[wave][l];
            s_before[wave][l] = total;
            total += here;
        }
        if (total == 0) status = 2;  // the reserved symbol alone: it never merged
        else if (bits[33] > 0) status = 1;
        if (status == 0) {
            // Annex K.3 figure K.3 as jchuff.c has it, then the reserved symbol out of the longest size in use
            for (int i = 32; i > 16; --i)
                while (bits[i] > 0) {
                    int j = i - 2;
                    while (j > 0 && bits[j] == 0) --j;
                    if (j == 0) { status = 1; bits[i] = 0; break; }  // not a prefix code's sizes: cannot come out of the merge
                    bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1;
                }
            int i = 16;
            while (i > 0 && bits[i] == 0) --i;
            if (i > 0) --bits[i];
        }
        if (status == 0) {
            int code = 0, rank = 0;
            for (int l = 1; l <= 16; ++l) {
                s_first_code[wave][l] = code, s_first_rank[wave][l] = rank;
                code = (code + bits[l]) << 1, rank += bits[l];
            }
            s_first_rank[wave][17] = rank;
            s_count[wave] = rank;
            if (frame_tables != nullptr && rank > ((wave & 1) ? 162 : 12)) status = 1;  // not a baseline table
        }
        s_status[wave] = status;
    }
    __syncthreads();
    const int status = s_status[wave];
    if (status == 0) {
        // libjpeg lists the symbols by their code size BEFORE the limiting, then by value; the limited counts then give
        // the listed symbols their final sizes in that order
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int index = lane + 64 * k;
            const int mine = size[k];
            if (mine == 0) continue;
            int rank = s_before[wave][mine];
            for (int j = 0; j < index; ++j) rank += s_size[wave][j] == mine;
            s_values[wave][rank] = (uint8_t)index;
        }
    }
    __syncthreads();
    if (status == 0) {
        for (int rank = lane; rank < s_count[wave]; rank += 64) {
            int l = 1;
            while (rank >= s_first_rank[wave][l + 1]) ++l;
            const int symbol = s_values[wave][rank];
            s_table[wave].code[symbol] = (uint16_t)(s_first_code[wave][l] + rank - s_first_rank[wave][l]);
            s_table[wave].size[symbol] = (uint8_t)l;
        }
    }
    __syncthreads();
    if (active) {
        if (lane < 16) out_bits[table * 16 + lane] = status == 0 ? (uint8_t)s_bits[wave][lane + 1] : 0;
        for (int i = lane; i < 256; i += 64) out_values[table * 256 + i] = status == 0 ? s_values[wave][i] : 0;
        if (lane == 0) out_status[table] = status;
    }
    if (frame_tables == nullptr || !active) return;
    const int64_t frame = blockIdx.x;
    const bool standard = (s_status[0] | s_status[1] | s_status[2] | s_status[3]) != 0;
    const HuffTable& view = wave == 0 ? kHuff.dc[0] : wave == 1 ? kHuff.ac[0] : wave == 2 ? kHuff.dc[1] : kHuff.ac[1];
    HuffTable* out_table = frame_tables + frame * kFrameTables + wave;
    for (int i = lane; i < 256; i += 64) {
        out_table->code[i] = standard ? view.code[i] : s_table[wave].code[i];
        out_table->size[i] = standard ? view.size[i] : s_table[wave].size[i];
    }
    int count = 0, before = 0;  // symbols of this table, DHT bytes of the frame's earlier tables
    for (int w = 0; w < kFrameTables; ++w) {
        int n = 0;
        if (standard)
            for (int i = 0; i < 16; ++i) n += kStandardDht.bits[w][i];
        else
            n = s_count[w];
        if (w < wave) before += 21 + n;
        if (w == wave) count = n;
    }
    uint8_t* dht = frame_dht + frame * kDhtCapacity + before;
    for (int i = lane; i < 21 + count; i += 64) {
        uint8_t byte;
        if (i == 0) byte = 0xFF;
        else if (i == 1) byte = 0xC4;
        else if (i == 2) byte = (uint8_t)((19 + count) >> 8);
        else if (i == 3) byte = (uint8_t)((19 + count) & 0xFF);
        else if (i == 4) byte = (uint8_t)(((wave & 1) << 4) | (wave >> 1));
        else if (i < 21) byte = standard ? kStandardDht.bits[wave][i - 5] : (uint8_t)s_bits[wave][i - 4];
        else byte = standard ? kStandardDht.values[wave][i - 21] : s_values[wave][i - 21];
        dht[i] = byte;
    }
    if (wave == kFrameTables - 1 && lane == 0) frame_dht_length[frame] = before + 21 + count;
}

// mjpeg_huffman_kernel with the frame's own tables, staged in LDS: a workgroup's blocks are all of one frame
__global__ void __launch_bounds__(256) mjpeg_huffman_frame_kernel(const int16_t* __restrict__ coef, int64_t mcu_cols, int64_t frame_blocks,
                                                                  int groups_per_frame, const HuffTable* __restrict__ frame_tables,
                                                                  uint32_t* __restrict__ bits, int* __restrict__ bit_counts) {
    __shared__ HuffTable tables[kFrameTables];
    const int64_t frame = blockIdx.x / groups_per_frame;
    const int64_t t = (int64_t)(blockIdx.x % groups_per_frame) * blockDim.x + threadIdx.x;
    const uint4* src = (const uint4*)(frame_tables + frame * kFrameTables);
    uint4* dst = (uint4*)tables;
    constexpr int kVectors = kFrameTables * (int)sizeof(HuffTable) / 16;
    for (int i = threadIdx.x; i < kVectors; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    if (t >= frame_blocks) return;
    const FrameBlock b = frame_block(coef, frame, t, mcu_cols, frame_blocks);
    bit_counts[b.g] = huffman_block(coef + b.g * 64, b.previous_dc, tables[2 * b.component], tables[2 * b.component + 1],
                                    bits + b.g * kBlockWords);
}

// ---- 3. one restart segment ----------------------------------------------------------------------------------------
// Bits [32 w, 32 w + 32) of the segment, given the blocks' bit offsets (offsets[n] = total): OR of the overlapping
// blocks' bits, then 1-padding past the end.
__host__ __device__ inline uint32_t segment_word(const uint32_t* __restrict__ bits, const int* __restrict__ offsets, int n, int w) {
    const int lo = 32 * w;
    // last block starting at or before `lo` (offsets strictly increase: a block has >= 4 bits, >= 2 with a frame's own tables)
    int a = 0, b = n - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (offsets[mid] <= lo) a = mid;
        else b = mid - 1;
    }
    uint32_t v = 0;
    for (int k = a; k < n && offsets[k] < lo + 32; ++k) {
        const uint32_t* s = bits + (size_t)k * kBlockWords;
        const int length = offsets[k + 1] - offsets[k];
        const int rel = lo - offsets[k];  // position of the word's first bit inside the block
        uint32_t part;
        int used;  // bits of the word, from its MSB, that the block's bits reach
        if (rel >= 0) {
            const int i = rel >> 5, sh = rel & 31;
            part = s[i] << sh;
            if (sh && (i + 1) * 32 < length) part |= s[i + 1] >> (32 - sh);
            used = length - rel;
        } else {
            part = s[0] >> (-rel);
            used = length - rel;
        }
        if (used < 32) part &= ~0u << (32 - used);
        v |= part;
    }
    const int remaining = offsets[n] - lo;
    if (remaining < 32) v |= ~0u >> remaining;
    return v;
}

template <typename T>
__device__ T block_exclusive_scan(T value, T* scratch, T* total) {
    const int tid = threadIdx.x;
    scratch[tid] = value;
    __syncthreads();
    for (int d = 1; d < kSegmentThreads; d <<= 1) {
        const T add = tid >= d ? scratch[tid - d] : 0;
        __syncthreads();
        scratch[tid] += add;
        __syncthreads();
    }
    const T inclusive = scratch[tid];
    *total = scratch[kSegmentThreads - 1];
    __syncthreads();
    return inclusive - value;
}

__global__ void __launch_bounds__(kSegmentThreads) mjpeg_segment_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ bit_counts,
                                                                        int segment_blocks, int64_t segment_capacity,
                                                                        uint8_t* __restrict__ slots, int* __restrict__ segment_sizes) {
    __shared__ int offsets[kMaxSegmentBlocks + 1];
    __shared__ int scratch[kSegmentThreads];
    const int64_t segment = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t* seg_bits = bits + segment * segment_blocks * kBlockWords;
    int carry = 0;
    for (int base = 0; base < segment_blocks; base += kSegmentThreads) {
        const int k = base + tid;
        const int count = k < segment_blocks ? bit_counts[segment * segment_blocks + k] : 0;
        int sum;
        const int before = block_exclusive_scan(count, scratch, &sum);
        if (k < segment_blocks) offsets[k] = carry + before;
        carry += sum;
    }
    if (tid == 0) offsets[segment_blocks] = carry;
    __syncthreads();
    const int total_bits = carry;
    const int bytes = (total_bits + 7) / 8, words = (bytes + 3) / 4;
    uint8_t* out = slots + segment * segment_capacity;
    int stuffed = 0;  // 0x00 bytes inserted before the current tile
    for (int base = 0; base < words; base += kSegmentThreads) {
        const int w = base + tid;
        uint32_t v = 0;
        int valid = 0, ff = 0;
        if (w < words) {
            v = segment_word(seg_bits, offsets, segment_blocks, w);
            valid = min(4, bytes - 4 * w);
            for (int j = 0; j < valid; ++j) ff += ((v >> (24 - 8 * j)) & 0xFF) == 0xFF;
        }
        int sum;
        int position = 4 * w + stuffed + block_exclusive_scan(ff, scratch, &sum);
        for (int j = 0; j < valid; ++j) {
            const uint8_t byte = (uint8_t)(v >> (24 - 8 * j));
            out[position++] = byte;
            if (byte == 0xFF) out[position++] = 0;
        }
        stuffed += sum;
    }
    if (tid == 0) segment_sizes[segment] = bytes + stuffed;
}

// ---- 4. frame layout and packing -----------------------------------------------------------------------------------
// One workgroup per frame: where each segment lands relative to its frame (a block scan of the segment sizes, each + 2
// for the RSTn or EOI after it), and the frame's size into offsets[frame + 1].
// kOwnTables (the optimised mode): header_bytes is the header without its DHT segments, dht_length[frame] their bytes.
template <bool kOwnTables>
__global__ void __launch_bounds__(kSegmentThreads) mjpeg_frame_layout_kernel(const int* __restrict__ segment_sizes, int mcu_rows,
                                                                              int header_bytes, const int* __restrict__ dht_length,
                                                                              int* __restrict__ segment_dst, int64_t* __restrict__ offsets) {
    __shared__ int scratch[kSegmentThreads];
    const int64_t frame = blockIdx.x;
    int carry = header_bytes;  // a frame is < 2^31 bytes: at most 1024 rows of < 850 000 bytes (side <= 8192)
    if (kOwnTables) carry += dht_length[frame];
    for (int base = 0; base < mcu_rows; base += kSegmentThreads) {
        const int r = base + threadIdx.x;
        const int size = r < mcu_rows ? segment_sizes[frame * mcu_rows + r] + 2 : 0;
        int sum;
        const int before = block_exclusive_scan(size, scratch, &sum);
        if (r < mcu_rows) segment_dst[frame * mcu_rows + r] = carry + before;
        carry += sum;
    }
    if (threadIdx.x == 0) offsets[frame + 1] = carry;
}

// One workgroup: the frame sizes in offsets[1 .. batch] scanned in place into the frames' positions, offsets[0] = 0.
__global__ void __launch_bounds__(kSegmentThreads) mjpeg_frame_offsets_kernel(int batch, int64_t* __restrict__ offsets) {
    __shared__ int64_t scratch[kSegmentThreads];
    int64_t carry = 0;
    for (int base = 0; base < batch; base += kSegmentThreads) {
        const int f = base + threadIdx.x;
        const int64_t size = f < batch ? offsets[f + 1] : 0;
        int64_t sum;
        const int64_t before = block_exclusive_scan(size, scratch, &sum);
        if (f < batch) offsets[f + 1] = carry + before + size;
        carry += sum;
    }
    if (threadIdx.x == 0) offsets[0] = 0;
}

// kOwnTables (the optimised mode): the header's DHT segments are the frame's, frame_dht [frames][kDhtCapacity] of
// dht_length[frame] bytes, between the parts of `header` in front of and behind its own.
template <bool kOwnTables>
__global__ void __launch_bounds__(256) mjpeg_pack_kernel(const uint8_t* __restrict__ slots, int64_t segment_capacity,
                                                         const int* __restrict__ segment_sizes, const int* __restrict__ segment_dst,
                                                         const int64_t* __restrict__ offsets, int mcu_rows, Header header,
                                                         const uint8_t* __restrict__ frame_dht, const int* __restrict__ dht_length,
                                                         uint8_t* __restrict__ out) {
    const int64_t segment = blockIdx.x;
    const int64_t frame = segment / mcu_rows;
    const int row = (int)(segment - frame * mcu_rows);
    const int size = segment_sizes[segment];
    const uint8_t* src = slots + segment * segment_capacity;
    uint8_t* dst = out + offsets[frame] + segment_dst[segment];
    for (int i = threadIdx.x; i < size; i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x == 0) {
        dst[size] = 0xFF;
        dst[size + 1] = row == mcu_rows - 1 ? 0xD9 : 0xD0 + (row & 7);
    }
    if (row == 0) {
        uint8_t* head = out + offsets[frame];
        if (kOwnTables) {
            const int own = dht_length[frame];
            const uint8_t* dht = frame_dht + frame * kDhtCapacity;
            for (int i = threadIdx.x; i < header.dht_begin; i += blockDim.x) head[i] = header.bytes[i];
            for (int i = threadIdx.x; i < own; i += blockDim.x) head[header.dht_begin + i] = dht[i];
            for (int i = threadIdx.x; i < header.length - header.dht_end; i += blockDim.x)
                head[header.dht_begin + own + i] = header.bytes[header.dht_end + i];
        } else {
            for (int i = threadIdx.x; i < header.length; i += blockDim.x) head[i] = header.bytes[i];
        }
    }
}

static int fail(int code, const std::string& message) { return gance::set_last_error(code, message); }

static int check_sizes(int32_t batch, int32_t side) {
    if (batch < 1) return fail(GANCE_ERR_INVALID_ARGUMENT, "batch must be >= 1");
    if (side < 16 || side > kMaxSide || side % 16 != 0)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "side must be a multiple of 16 in [16, " + std::to_string(kMaxSide) + "], got " +
                                                    std::to_string(side));
    return GANCE_OK;
}

static int check_rect_sizes(int32_t batch, int32_t width, int32_t height) {
    if (batch < 1) return fail(GANCE_ERR_INVALID_ARGUMENT, "batch must be >= 1");
    for (const int32_t extent : {width, height})
        if (extent < 16 || extent > kMaxSide || extent % 16 != 0)
            return fail(GANCE_ERR_INVALID_ARGUMENT, "width and height must be multiples of 16 in [16, " + std::to_string(kMaxSide) +
                                                        "], got " + std::to_string(width) + " x " + std::to_string(height));
    return GANCE_OK;
}

// The encode of `batch` frames [height][width][3]; sizes, quality and pointers (NULL) are checked by the callers.
static int encode(const char* entry, const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, int32_t quality,
                  void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets,
                  void* stream_ptr, bool optimized = false) {
    if (quality < 1 || quality > 100) return fail(GANCE_ERR_INVALID_ARGUMENT, "quality must be in [1, 100], got " + std::to_string(quality));
    if ((uintptr_t)d_frames % 16 != 0 || (uintptr_t)d_workspace % 16 != 0)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "frames and workspace must be 16-byte aligned");
    const Layout l = layout_of(batch, width, height, optimized);
    const std::string bounds = std::string(" needed (") + entry + ")";
    if (workspace_bytes < (uint64_t)l.workspace_bytes)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                                    std::to_string(l.workspace_bytes) + bounds);
    if (out_capacity < (uint64_t)l.out_capacity)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "output capacity of " + std::to_string(out_capacity) + " bytes, " +
                                                    std::to_string(l.out_capacity) + bounds);
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return fail(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    gance::DeviceGuard guard(gance::device_of_pointer(d_frames));  // launch where the frames live
    if (guard.status() != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));

    char* ws = (char*)d_workspace;
    int16_t* coef = (int16_t*)ws;
    uint32_t* bits = (uint32_t*)(ws + l.coef_bytes);
    int* bit_counts = (int*)(ws + l.coef_bytes + l.bits_bytes);
    uint8_t* slots = (uint8_t*)(ws + l.coef_bytes + l.bits_bytes + l.bitlen_bytes);
    int* segment_sizes = (int*)(ws + l.coef_bytes + l.bits_bytes + l.bitlen_bytes + l.slot_bytes);
    int* segment_dst = (int*)(ws + l.coef_bytes + l.bits_bytes + l.bitlen_bytes + l.slot_bytes + l.size_bytes);
    const Header header = make_header(width, height, quality);
    hipStream_t stream = (hipStream_t)stream_ptr;
    const unsigned grid = (unsigned)((l.blocks + 255) / 256);
    mjpeg_transform_kernel<<<grid, 256, 0, stream>>>(d_frames, width, height, l.mcu_rows, l.mcu_cols, l.blocks, make_quant(quality), coef);
    if (!optimized) {
        mjpeg_huffman_kernel<<<grid, 256, 0, stream>>>(coef, l.mcu_cols, l.blocks, bits, bit_counts);
        mjpeg_segment_kernel<<<(unsigned)l.segments, kSegmentThreads, 0, stream>>>(bits, bit_counts, (int)l.segment_blocks, l.segment_capacity,
                                                                                   slots, segment_sizes);
        mjpeg_frame_layout_kernel<false><<<(unsigned)batch, kSegmentThreads, 0, stream>>>(segment_sizes, (int)l.mcu_rows, header.length, nullptr,
                                                                                          segment_dst, d_offsets);
        mjpeg_frame_offsets_kernel<<<1, kSegmentThreads, 0, stream>>>(batch, d_offsets);
        mjpeg_pack_kernel<false><<<(unsigned)l.segments, 256, 0, stream>>>(slots, l.segment_capacity, segment_sizes, segment_dst, d_offsets,
                                                                           (int)l.mcu_rows, header, nullptr, nullptr, d_out);
    } else {
        char* own = (char*)(segment_dst) + l.dst_bytes;
        int* counts = (int*)own;
        HuffTable* frame_tables = (HuffTable*)(own + l.count_bytes);
        uint8_t* frame_dht = (uint8_t*)(own + l.count_bytes + l.table_bytes);
        int* dht_length = (int*)(own + l.count_bytes + l.table_bytes + l.dht_bytes);
        uint8_t* table_bits = (uint8_t*)(own + l.count_bytes + l.table_bytes + l.dht_bytes + l.dht_length_bytes);
        uint8_t* table_values = table_bits + l.table_bits_bytes;
        int* table_status = (int*)(table_values + l.table_values_bytes);
        const int64_t frame_blocks = l.blocks / batch;
        const int groups_per_frame = (int)((frame_blocks + 255) / 256);
        const unsigned frame_grid = (unsigned)(batch * (int64_t)groups_per_frame);
        const hipError_t zeroed = hipMemsetAsync(counts, 0, (size_t)l.count_bytes, stream);
        if (zeroed != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(zeroed));
        mjpeg_symbol_count_kernel<<<frame_grid, 256, 0, stream>>>(coef, l.mcu_cols, frame_blocks, groups_per_frame, counts);
        mjpeg_optimal_tables_kernel<<<(unsigned)batch, kTableThreads, 0, stream>>>(counts, (int64_t)batch * kFrameTables, table_bits, table_values,
                                                                                   table_status, frame_tables, frame_dht, dht_length);
        mjpeg_huffman_frame_kernel<<<frame_grid, 256, 0, stream>>>(coef, l.mcu_cols, frame_blocks, groups_per_frame, frame_tables, bits,
                                                                   bit_counts);
        mjpeg_segment_kernel<<<(unsigned)l.segments, kSegmentThreads, 0, stream>>>(bits, bit_counts, (int)l.segment_blocks, l.segment_capacity,
                                                                                   slots, segment_sizes);
        mjpeg_frame_layout_kernel<true><<<(unsigned)batch, kSegmentThreads, 0, stream>>>(
            segment_sizes, (int)l.mcu_rows, header.length - (header.dht_end - header.dht_begin), dht_length, segment_dst, d_offsets);
        mjpeg_frame_offsets_kernel<<<1, kSegmentThreads, 0, stream>>>(batch, d_offsets);
        mjpeg_pack_kernel<true><<<(unsigned)l.segments, 256, 0, stream>>>(slots, l.segment_capacity, segment_sizes, segment_dst, d_offsets,
                                                                          (int)l.mcu_rows, header, frame_dht, dht_length, d_out);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("mjpeg launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

}  // namespace gance_mjpeg

extern "C" {

int gance_jpeg_encode_rect_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes, uint64_t* out_capacity) {
    using namespace gance_mjpeg;
    if (workspace_bytes == nullptr || out_capacity == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_jpeg_encode_rect_bounds");
    if (const int status = check_rect_sizes(batch, width, height)) return status;
    const Layout l = layout_of(batch, width, height);
    *workspace_bytes = (uint64_t)l.workspace_bytes;
    *out_capacity = (uint64_t)l.out_capacity;
    return GANCE_OK;
}

int gance_jpeg_encode_rect_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, int32_t quality, void* d_workspace,
                              uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets, void* stream_ptr) {
    using namespace gance_mjpeg;
    if (d_frames == nullptr || d_workspace == nullptr || d_out == nullptr || d_offsets == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_jpeg_encode_rect_u8");
    if (const int status = check_rect_sizes(batch, width, height)) return status;
    return encode("gance_jpeg_encode_rect_bounds", d_frames, batch, width, height, quality, d_workspace, workspace_bytes, d_out,
                  out_capacity, d_offsets, stream_ptr);
}

int gance_jpeg_encode_bounds(int32_t batch, int32_t side, uint64_t* workspace_bytes, uint64_t* out_capacity) {
    using namespace gance_mjpeg;
    if (workspace_bytes == nullptr || out_capacity == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_jpeg_encode_bounds");
    if (const int status = check_sizes(batch, side)) return status;
    const Layout l = layout_of(batch, side, side);
    *workspace_bytes = (uint64_t)l.workspace_bytes;
    *out_capacity = (uint64_t)l.out_capacity;
    return GANCE_OK;
}

int gance_jpeg_encode_u8(const uint8_t* d_frames, int32_t batch, int32_t side, int32_t quality, void* d_workspace,
                         uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets, void* stream_ptr) {
    using namespace gance_mjpeg;
    if (d_frames == nullptr || d_workspace == nullptr || d_out == nullptr || d_offsets == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_jpeg_encode_u8");
    if (const int status = check_sizes(batch, side)) return status;
    return encode("gance_jpeg_encode_bounds", d_frames, batch, side, side, quality, d_workspace, workspace_bytes, d_out, out_capacity,
                  d_offsets, stream_ptr);
}

int gance_jpeg_encode_rect_optimized_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes,
                                            uint64_t* out_capacity) {
    using namespace gance_mjpeg;
    if (workspace_bytes == nullptr || out_capacity == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_jpeg_encode_rect_optimized_bounds");
    if (const int status = check_rect_sizes(batch, width, height)) return status;
    const Layout l = layout_of(batch, width, height, true);
    *workspace_bytes = (uint64_t)l.workspace_bytes;
    *out_capacity = (uint64_t)l.out_capacity;
    return GANCE_OK;
}

int gance_jpeg_encode_rect_optimized_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, int32_t quality,
                                        void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                        int64_t* d_offsets, void* stream_ptr) {
    using namespace gance_mjpeg;
    if (d_frames == nullptr || d_workspace == nullptr || d_out == nullptr || d_offsets == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_jpeg_encode_rect_optimized_u8");
    if (const int status = check_rect_sizes(batch, width, height)) return status;
    return encode("gance_jpeg_encode_rect_optimized_bounds", d_frames, batch, width, height, quality, d_workspace, workspace_bytes, d_out,
                  out_capacity, d_offsets, stream_ptr, true);
}

int gance_jpeg_optimal_tables(const int32_t* d_counts, int32_t n, uint8_t* d_bits, uint8_t* d_values, int32_t* d_status,
                              void* stream_ptr) {
    using namespace gance_mjpeg;
    if (d_counts == nullptr || d_bits == nullptr || d_values == nullptr || d_status == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_jpeg_optimal_tables");
    if (n < 1) return fail(GANCE_ERR_INVALID_ARGUMENT, "n must be >= 1, got " + std::to_string(n));
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return fail(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    gance::DeviceGuard guard(gance::device_of_pointer(d_counts));
    if (guard.status() != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));
    const unsigned grid = (unsigned)(((int64_t)n + kFrameTables - 1) / kFrameTables);
    mjpeg_optimal_tables_kernel<<<grid, kTableThreads, 0, (hipStream_t)stream_ptr>>>(d_counts, n, d_bits, d_values, d_status, nullptr, nullptr,
                                                                                    nullptr);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("mjpeg tables launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

}  // extern "C"
