// What the two PNG encoders share (png.hip: literal-only Huffman; png_lz.hip: the same with a match search): the CRC
// helpers, the code builders and the bit writer, the filter, literal-only segment, layout, offsets and pack kernels, the
// sizes of a call and its argument checks. Kernels and device tables have internal linkage: each of the two files
// carries its own.
//
//   filter     one byte per row + 3 * width filtered bytes. The row's filter is the one of None / Sub / Up / Average /
//              Paeth (bpp 3, zeros above row 0 and left of column 0) with the smallest sum of |int8(byte)|, ties to the
//              lowest number: libpng's minimum-sum-of-absolutes heuristic.
//   deflate    the frame's filtered stream in independent segments of kSegmentBytes. A segment is one dynamic-Huffman
//              block over literals and end-of-block (no match search), its code lengths built from the segment's own
//              histogram (minimum redundancy, limited to 15 bits), followed by an empty stored block that ends it on a
//              byte boundary (a sync flush); or one stored block whenever that is not larger. The last segment's final
//              block carries BFINAL.
//   container  signature, IHDR, one IDAT chunk per segment (the zlib header in front of the first), one 4-byte IDAT
//              chunk with the Adler-32 of the whole filtered stream, IEND. Every chunk CRC covers bytes one workgroup made.
//
// Four launches on the caller's stream, deterministic (integer LDS atomics only, no workgroup waits on another):
//   1. png_filter_kernel    one workgroup per row: the five sums, the choice, the filtered row into the workspace
//   2. png_segment_kernel   one workgroup per segment: histogram, code lengths, header, bits, CRC -> its slot; its
//                           Adler-32 sums
//   3. png_layout_kernel    one workgroup per frame: scan of the slot sizes, the frame's Adler-32, its size; then
//      png_offsets_kernel   the scan of the frame sizes
//   4. png_pack_kernel      one workgroup per segment: slot -> output; header and trailer chunks
// A frame of one flat colour costs about 1 bit per byte (a literal code is at least 1 bit): see DESIGN.md.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace gance_png {

constexpr int kMaxSide = 8192;
constexpr int kSegmentBytes = 32768;  // hip_lib.PNG_SEGMENT_BYTES; <= 65535 so that a segment fits one stored block
constexpr int kThreads = 256;
constexpr int kChunkBytes = kSegmentBytes / kThreads;  // filtered bytes per thread of the segment kernel
constexpr int kLiterals = 257;                         // 256 byte values + end-of-block
constexpr int kMaxLitBits = 15, kMaxClBits = 7;
constexpr int kHeadBytes = 8 + 25;  // signature + IHDR chunk
constexpr int kTailBytes = 16 + 12;  // Adler-32 IDAT chunk + IEND chunk
// type + zlib header + stored-block header + data + CRC; the coded form is used only when it is not larger than the stored
constexpr int kBufferBytes = 4 + 2 + 5 + kSegmentBytes + 4;
constexpr int kBufferWords = (kBufferBytes + 3) / 4 + 2;
static_assert(kChunkBytes % 16 == 0, "a thread reads its bytes as 16-byte words");

__host__ __device__ constexpr uint32_t crc_table_entry(uint32_t n) {
    uint32_t c = n;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}
struct CrcTable {
    uint32_t v[256];
};
constexpr CrcTable make_crc_table() {
    CrcTable t{};
    for (uint32_t n = 0; n < 256; ++n) t.v[n] = crc_table_entry(n);
    return t;
}
static __constant__ CrcTable kCrcTable = make_crc_table();
static constexpr CrcTable kHostCrcTable = make_crc_table();

// a(x) b(x) mod the CRC-32 polynomial, reflected representation (x^0 is bit 31)
__host__ __device__ inline uint32_t crc_multiply(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// x^(8 n) mod the polynomial: the operator that appends n bytes to a CRC (crc(A B) = crc(A) x^(8 |B|) + crc(B))
__host__ __device__ inline uint32_t crc_shift_of_bytes(uint32_t n) {
    uint32_t result = 0x80000000u, power = 0x00800000u;  // 1, x^8
    while (n) {
        if (n & 1) result = crc_multiply(power, result);
        power = crc_multiply(power, power);
        n >>= 1;
    }
    return result;
}

static uint32_t host_crc(const uint8_t* bytes, int n) {
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) c = kHostCrcTable.v[(c ^ bytes[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// ---- sizes ---------------------------------------------------------------------------------------------------------
struct Layout {
    int64_t row_bytes, stream_bytes, stream_stride, segments, last_segment_bytes;
    int64_t slot_capacity;
    int64_t stream_total, slot_total, size_total, dst_total, adler_total;
    int64_t workspace_bytes, frame_capacity, out_capacity;
};

static int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

static Layout layout_of(int64_t batch, int64_t width, int64_t height) {
    Layout l{};
    l.row_bytes = 3 * width + 1;
    l.stream_bytes = height * l.row_bytes;
    l.stream_stride = round16(l.stream_bytes);
    l.segments = (l.stream_bytes + kSegmentBytes - 1) / kSegmentBytes;
    l.last_segment_bytes = l.stream_bytes - (l.segments - 1) * kSegmentBytes;
    l.slot_capacity = round16(4 + kBufferWords * 4);
    l.stream_total = batch * l.stream_stride;
    l.slot_total = batch * l.segments * l.slot_capacity;
    l.size_total = round16(batch * l.segments * 4);
    l.dst_total = round16(batch * l.segments * 4);
    l.adler_total = round16(batch * l.segments * 8) + round16(batch * 4);
    l.workspace_bytes = l.stream_total + l.slot_total + l.size_total + l.dst_total + l.adler_total;
    // every segment stored: 12 bytes of chunk + 5 of block header around its bytes, the zlib header once
    l.frame_capacity = kHeadBytes + 2 + 17 * l.segments + l.stream_bytes + kTailBytes;
    l.out_capacity = batch * l.frame_capacity;
    return l;
}

// ---- 1. filter -----------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__host__ __device__ __forceinline__ int filtered_byte(int filter, int x, int a, int b, int c) {
    switch (filter) {
        case 0: return x;
        case 1: return (x - a) & 0xFF;
        case 2: return (x - b) & 0xFF;
        case 3: return (x - ((a + b) >> 1)) & 0xFF;
        default: return (x - paeth(a, b, c)) & 0xFF;
    }
}

__host__ __device__ __forceinline__ int magnitude(int v) { return v < 128 ? v : 256 - v; }

static __global__ void __launch_bounds__(kThreads) png_filter_kernel(const uint8_t* __restrict__ frames, int width, int height,
                                                              int64_t stream_stride, uint8_t* __restrict__ streams) {
    __shared__ uint32_t sums[5][kThreads];
    const int64_t frame = blockIdx.x / height;
    const int row = (int)(blockIdx.x - frame * height);
    const int n = 3 * width;
    const int tid = threadIdx.x;
    const uint8_t* current = frames + (frame * height + row) * (int64_t)n;
    const uint8_t* above = current - n;  // read only when row > 0
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += kThreads) {
        const int x = current[i];
        const int a = i >= 3 ? current[i - 3] : 0;
        const int b = row > 0 ? above[i] : 0;
        const int c = (row > 0 && i >= 3) ? above[i - 3] : 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) sum[f] += (uint32_t)magnitude(filtered_byte(f, x, a, b, c));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) sums[f][tid] = sum[f];
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
#pragma unroll
            for (int f = 0; f < 5; ++f) sums[f][tid] += sums[f][tid + d];
        }
        __syncthreads();
    }
    int filter = 0;
    uint32_t best = sums[0][0];  // a row is at most 24576 bytes of at most 128: no overflow
#pragma unroll
    for (int f = 1; f < 5; ++f)
        if (sums[f][0] < best) best = sums[f][0], filter = f;
    uint8_t* out = streams + frame * stream_stride + (int64_t)row * (n + 1);
    if (tid == 0) out[0] = (uint8_t)filter;
    for (int i = tid; i < n; i += kThreads) {
        const int x = current[i];
        const int a = i >= 3 ? current[i - 3] : 0;
        const int b = row > 0 ? above[i] : 0;
        const int c = (row > 0 && i >= 3) ? above[i - 3] : 0;
        out[1 + i] = (uint8_t)filtered_byte(filter, x, a, b, c);
    }
}

// ---- 2. one segment --------------------------------------------------------------------------------------------------
template <typename T>
__device__ T block_exclusive_scan(T value, T* scratch, T* total) {
    const int tid = threadIdx.x;
    scratch[tid] = value;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const T add = tid >= d ? scratch[tid - d] : 0;
        __syncthreads();
        scratch[tid] += add;
        __syncthreads();
    }
    const T inclusive = scratch[tid];
    *total = scratch[kThreads - 1];
    __syncthreads();
    return inclusive - value;
}

// Code lengths of a minimum-redundancy code limited to `max_bits`, for `n` >= 2 symbols given by ascending frequency:
// a[i] is the i-th smallest frequency on entry (Moffat and Katajainen's in-place calculation), symbols[i] its symbol;
// lengths[symbol] receives the length. Symbols not listed keep their length (0). One thread.
__host__ __device__ inline void limited_code_lengths(uint32_t* a, const uint16_t* symbols, int n, int max_bits, uint8_t* lengths) {
    if (n == 2) {
        a[0] = a[1] = 1;
    } else {
        a[0] += a[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < n - 1; ++next) {
            if (leaf >= n || a[root] < a[leaf]) {
                a[next] = a[root];
                a[root++] = (uint32_t)next;
            } else {
                a[next] = a[leaf++];
            }
            if (leaf >= n || (root < next && a[root] < a[leaf])) {
                a[next] += a[root];
                a[root++] = (uint32_t)next;
            } else {
                a[next] += a[leaf++];
            }
        }
        a[n - 2] = 0;
        for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
        int available = 1, used = 0, depth = 0;
        root = n - 2;
        int next = n - 1;
        while (available > 0) {
            while (root >= 0 && (int)a[root] == depth) {
                ++used;
                --root;
            }
            while (available > used) {
                a[next--] = (uint32_t)depth;
                --available;
            }
            available = 2 * used;
            ++depth;
            used = 0;
        }
    }
    // codes per length, the over-long ones moved to max_bits, then the Kraft sum brought back to one
    int count[40];
    for (int i = 0; i < 40; ++i) count[i] = 0;
    for (int i = 0; i < n; ++i) ++count[a[i] < 39 ? a[i] : 39];
    for (int i = max_bits + 1; i < 40; ++i) count[max_bits] += count[i];
    uint32_t total = 0;
    for (int i = max_bits; i > 0; --i) total += (uint32_t)count[i] << (max_bits - i);
    while (total != (1u << max_bits)) {
        --count[max_bits];
        for (int i = max_bits - 1; i > 0; --i)
            if (count[i]) {
                --count[i];
                count[i + 1] += 2;
                break;
            }
        --total;
    }
    // the most frequent symbols take the shortest codes
    int j = n;
    for (int length = 1; length <= max_bits; ++length)
        for (int k = count[length]; k > 0; --k) lengths[symbols[--j]] = (uint8_t)length;
}

// Canonical codes (RFC 1951 3.2.2) of `lengths`, bit-reversed for deflate's LSB-first packing. One thread.
__host__ __device__ inline void canonical_codes(const uint8_t* lengths, int n, int max_bits, uint16_t* codes) {
    int count[16], next[16];
    for (int i = 0; i < 16; ++i) count[i] = 0;
    for (int s = 0; s < n; ++s) ++count[lengths[s]];
    count[0] = 0;
    int code = 0;
    next[0] = 0;
    for (int bits = 1; bits <= max_bits; ++bits) {
        code = (code + count[bits - 1]) << 1;
        next[bits] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int length = lengths[s];
        if (length == 0) {
            codes[s] = 0;
            continue;
        }
        uint32_t v = (uint32_t)next[length]++, r = 0;
        for (int i = 0; i < length; ++i) r |= ((v >> i) & 1u) << (length - 1 - i);
        codes[s] = (uint16_t)r;
    }
}

// Bits into a zeroed word buffer, LSB first; other threads may own the other bits of a word, so words are OR-ed in
struct BitWriter {
    uint32_t* words;
    uint64_t acc = 0;
    int pending, word;
    __host__ __device__ BitWriter(uint32_t* buffer, int bit_position) : words(buffer), pending(bit_position & 31), word(bit_position >> 5) {}
    __host__ __device__ __forceinline__ void merge(uint32_t* target, uint32_t bits) {
#ifdef __HIP_DEVICE_COMPILE__
        atomicOr(target, bits);
#else
        *target |= bits;
#endif
    }
    __host__ __device__ __forceinline__ void put(uint32_t bits, int size) {  // size <= 16
        acc |= (uint64_t)bits << pending;
        pending += size;
        if (pending >= 32) {
            merge(&words[word++], (uint32_t)acc);
            acc >>= 32;
            pending -= 32;
        }
    }
    __host__ __device__ __forceinline__ void finish() {
        if (pending > 0) merge(&words[word], (uint32_t)acc);
    }
};

__host__ __device__ __forceinline__ int cl_order(int i) {  // RFC 1951 3.2.7: the order the code-length code lengths are sent in
    constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// The code-length code (limited to 7 bits) of a block header whose code-length symbols occur cl_frequency[0 .. 18] times:
// its lengths and codes, the number of lengths sent (HCLEN + 4) in *cl_count; returns the bits of those lengths (3 each)
// plus the bits of the symbols' codes (extra bits of 16 / 17 / 18 not counted). One thread.
__host__ __device__ inline uint32_t code_length_code(const uint32_t* cl_frequency, uint8_t* cl_length, uint16_t* cl_code, int* cl_count_out) {
    uint16_t cl_symbol[19];
    uint8_t cl_len[19];
    uint16_t cl_cod[19];
    for (int i = 0; i < 19; ++i) cl_len[i] = 0;
    int cl_used = 0;
    for (int s = 0; s < 19; ++s)
        if (cl_frequency[s] > 0) cl_symbol[cl_used++] = (uint16_t)s;
    for (int i = 1; i < cl_used; ++i)  // insertion sort by (frequency, symbol)
        for (int j = i; j > 0 && cl_frequency[cl_symbol[j]] < cl_frequency[cl_symbol[j - 1]]; --j) {
            const uint16_t t = cl_symbol[j];
            cl_symbol[j] = cl_symbol[j - 1];
            cl_symbol[j - 1] = t;
        }
    uint32_t cl_sorted[19];
    for (int i = 0; i < cl_used; ++i) cl_sorted[i] = cl_frequency[cl_symbol[i]];
    uint32_t bits = 0;
    if (cl_used >= 2) {  // always: the lengths of 257 or more symbols cannot all be equal, and two used symbols leave zeros
        limited_code_lengths(cl_sorted, cl_symbol, cl_used, kMaxClBits, cl_len);
    } else {
        cl_len[cl_symbol[0]] = 1;
        cl_len[cl_symbol[0] == 0 ? 1 : 0] = 1;
    }
    canonical_codes(cl_len, 19, kMaxClBits, cl_cod);
    int cl_count = 19;
    while (cl_count > 4 && cl_len[cl_order(cl_count - 1)] == 0) --cl_count;
    bits += 3 * cl_count;
    for (int s = 0; s < 19; ++s) bits += cl_frequency[s] * cl_len[s];
    for (int s = 0; s < 19; ++s) cl_length[s] = cl_len[s], cl_code[s] = cl_cod[s];
    *cl_count_out = cl_count;
    return bits;
}

// What thread 0 decides for the workgroup
struct SegmentPlan {
    int coded;        // 1: dynamic block + empty stored block; 0: one stored block
    int data_bit;     // position of the first literal's code in the buffer
    int total_bytes;  // chunk type + data
    int cl_count;     // code-length code lengths sent (HCLEN + 4)
};

// The literal code of a segment from its histogram (end-of-block counted) and its used symbols in ascending (frequency,
// symbol) order (sorted_frequency is consumed), the code-length code of the block header, and the choice between the
// coded and the stored form. One thread.
__host__ __device__ inline SegmentPlan plan_segment(const uint32_t* histogram, uint32_t* sorted_frequency, const uint16_t* sorted_symbol,
                                                    int used_symbols, int n, int start_bytes, uint8_t* lit_length, uint16_t* lit_code,
                                                    uint8_t* cl_length, uint16_t* cl_code) {
    SegmentPlan plan;
    // literal code: at least two symbols (a byte and end-of-block), so the code is complete
    limited_code_lengths(sorted_frequency, sorted_symbol, used_symbols, kMaxLitBits, lit_length);
    canonical_codes(lit_length, kLiterals, kMaxLitBits, lit_code);
    uint32_t data_bits = 0;
    for (int s = 0; s < kLiterals; ++s) data_bits += histogram[s] * lit_length[s];  // end-of-block included
    // code-length code over the 257 literal lengths and the one distance length (1), no repeat symbols
    uint32_t cl_frequency[19];
    for (int i = 0; i < 19; ++i) cl_frequency[i] = 0;
    for (int s = 0; s < kLiterals; ++s) ++cl_frequency[lit_length[s]];
    ++cl_frequency[1];
    int cl_count;
    const uint32_t header_bits = 3 + 5 + 5 + 4 + code_length_code(cl_frequency, cl_length, cl_code, &cl_count);
    // coded: header, literals, end-of-block, then the 3 bits of an empty stored block, padding, 00 00 FF FF
    const uint32_t coded_bits = header_bits + data_bits + 3;
    const int coded_bytes = (int)((coded_bits + 7) / 8) + 4;
    const int stored_bytes = 5 + n;
    plan.coded = coded_bytes <= stored_bytes ? 1 : 0;
    plan.data_bit = 8 * start_bytes + (int)header_bits;
    plan.total_bytes = start_bytes + (plan.coded ? coded_bytes : stored_bytes);
    plan.cl_count = cl_count;
    return plan;
}

// End-of-block at eob_bit and the empty stored block that ends the segment on a byte boundary. One thread.
__host__ __device__ inline void write_block_tail(uint32_t* buffer, int eob_bit, uint32_t eob_code, int eob_length, bool last) {
    BitWriter tail(buffer, eob_bit);
    tail.put(eob_code, eob_length);
    tail.put(last ? 1 : 0, 1);  // BFINAL of the empty stored block
    tail.put(0, 2);
    tail.put(0, (8 - ((eob_bit + eob_length + 3) & 7)) & 7);  // to the byte boundary
    tail.put(0, 16);                                          // LEN = 0
    tail.put(0xFFFF, 16);                                     // NLEN
    tail.finish();
}

// The dynamic block's header in front of the literals' codes, and behind them (all_bits of them) end-of-block and the
// empty stored block. One thread.
__host__ __device__ inline void write_head_and_tail(uint32_t* buffer, const SegmentPlan& plan, int start_bytes, int all_bits, bool last,
                                                    const uint8_t* lit_length, const uint16_t* lit_code, const uint8_t* cl_length,
                                                    const uint16_t* cl_code) {
    BitWriter head(buffer, 8 * start_bytes);
    head.put(0, 1);  // BFINAL
    head.put(2, 2);  // BTYPE: dynamic Huffman codes
    head.put(0, 5);  // HLIT: 257 literal / length codes
    head.put(0, 5);  // HDIST: one distance code
    head.put((uint32_t)(plan.cl_count - 4), 4);
    for (int i = 0; i < plan.cl_count; ++i) head.put(cl_length[cl_order(i)], 3);
    for (int s = 0; s < kLiterals; ++s) head.put(cl_code[lit_length[s]], cl_length[lit_length[s]]);
    head.put(cl_code[1], cl_length[1]);  // the distance code: one code of one bit (RFC 1951 3.2.7)
    head.finish();
    write_block_tail(buffer, plan.data_bit + (int)all_bits, lit_code[256], lit_length[256], last);
}

// CRC-32 of the chunk's type and data in `buffer` (total bytes), appended to it; then the chunk into its slot: the length
// of the data (big endian), type, data, CRC, and the slot's size. The whole workgroup; the caller has synchronised after
// the last write to the buffer. The thread's piece, pieces of one length laid against the END of the bytes (so only left
// pieces are short or empty), then a tree of crc(A B) = crc(A) x^(8 |B|) + crc(B).
__device__ __forceinline__ void crc_and_store_slot(uint32_t* buffer, int total, const uint32_t* crc_table, uint32_t* scratch,
                                                   uint8_t* __restrict__ slots, int64_t slot_capacity, int* __restrict__ slot_sizes) {
    const int tid = threadIdx.x;
    uint8_t* bytes = (uint8_t*)buffer;
    const int piece = (total + kThreads - 1) / kThreads;
    {
        const int piece_end = total - (kThreads - 1 - tid) * piece;
        const int piece_begin = max(piece_end - piece, 0);
        uint32_t c = 0;
        if (piece_end > 0) {
            c = 0xFFFFFFFFu;
            for (int i = piece_begin; i < piece_end; ++i) c = crc_table[(c ^ bytes[i]) & 0xFF] ^ (c >> 8);
            c ^= 0xFFFFFFFFu;
        }
        scratch[tid] = c;
    }
    uint32_t shift = crc_shift_of_bytes((uint32_t)piece);
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        if (tid % (2 * d) == 0) scratch[tid] = crc_multiply(shift, scratch[tid]) ^ scratch[tid + d];
        shift = crc_multiply(shift, shift);
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t crc = scratch[0];
        bytes[total] = (uint8_t)(crc >> 24);
        bytes[total + 1] = (uint8_t)(crc >> 16);
        bytes[total + 2] = (uint8_t)(crc >> 8);
        bytes[total + 3] = (uint8_t)crc;
    }
    __syncthreads();
    uint32_t* slot = (uint32_t*)(slots + (int64_t)blockIdx.x * slot_capacity);
    const int words = (total + 4 + 3) / 4;  // <= kBufferWords
    for (int i = tid; i < words; i += kThreads) slot[1 + i] = buffer[i];
    if (tid == 0) {
        slot[0] = __builtin_bswap32((uint32_t)(total - 4));
        slot_sizes[blockIdx.x] = total + 8;
    }
}

static __global__ void __launch_bounds__(kThreads) png_segment_kernel(const uint8_t* __restrict__ streams, int64_t stream_stride, int64_t stream_bytes,
                                                               int segments, int64_t slot_capacity, uint8_t* __restrict__ slots,
                                                               int* __restrict__ slot_sizes, uint32_t* __restrict__ adler_sums) {
    __shared__ uint32_t buffer[kBufferWords];  // the chunk from its type on: "IDAT", data, CRC
    __shared__ uint32_t histogram[kLiterals + 3];
    __shared__ uint32_t sorted_frequency[kLiterals + 3];
    __shared__ uint16_t sorted_symbol[kLiterals + 3];
    __shared__ uint8_t lit_length[kLiterals + 3];
    __shared__ uint16_t lit_code[kLiterals + 3];
    __shared__ uint8_t cl_length[19];
    __shared__ uint16_t cl_code[19];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t scratch[kThreads];
    __shared__ uint32_t scratch2[kThreads];
    __shared__ int used_symbols;
    __shared__ SegmentPlan plan;

    const int tid = threadIdx.x;
    const int64_t frame = blockIdx.x / segments;
    const int segment = (int)(blockIdx.x - frame * segments);
    const bool first = segment == 0, last = segment == segments - 1;
    const int n = (int)min((int64_t)kSegmentBytes, stream_bytes - (int64_t)segment * kSegmentBytes);  // >= 1
    const uint8_t* src = streams + frame * stream_stride + (int64_t)segment * kSegmentBytes;          // 16-byte aligned
    const int start_bytes = first ? 6 : 4;  // chunk type, zlib header

    for (int i = tid; i < kBufferWords; i += kThreads) buffer[i] = 0;
    for (int i = tid; i < kLiterals + 3; i += kThreads) histogram[i] = 0, lit_length[i] = 0;
    crc_table[tid] = kCrcTable.v[tid];
    if (tid == 0) used_symbols = 0;
    __syncthreads();

    // this thread's bytes: [begin, end) of the segment
    const int begin = min(tid * kChunkBytes, n), end = min(begin + kChunkBytes, n);
    uint32_t adler_a = 0, adler_b = 0;  // sum of the bytes, sum of (end - position) * byte: at most 128 * 128 * 255
    for (int base = begin; base < end; base += 16) {
        const uint4 v = *(const uint4*)(src + base);  // inside the frame's stream_stride bytes
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (base + k < end) {
                const uint32_t byte = (w[k >> 2] >> (8 * (k & 3))) & 0xFF;
                atomicAdd(&histogram[byte], 1u);
                adler_a += byte;
                adler_b += (uint32_t)(end - (base + k)) * byte;
            }
        }
    }
    if (tid == 0) {
        histogram[256] = 1;  // end-of-block
        buffer[0] = 0x54414449u;  // "IDAT"
        if (first) buffer[1] = 0x0178u;  // zlib header: deflate, 32 KiB window, no dictionary, fastest (0x78 0x01)
    }
    // Adler-32 sums of the segment as if it began at (0, 0): A = sum of bytes, B = sum of (n - position) * byte, mod 65521
    {
        const uint32_t after = (uint32_t)(n - end);  // bytes of the segment behind this thread's
        const uint32_t b_here = (adler_b + (adler_a * after) % 65521u) % 65521u;  // 32640 * 32768 < 2^32
        uint32_t total_a, total_b;
        block_exclusive_scan(adler_a, scratch, &total_a);  // at most 32768 * 255
        block_exclusive_scan(b_here, scratch2, &total_b);  // at most 256 * 65520
        if (tid == 0) {
            adler_sums[2 * (int64_t)blockIdx.x] = total_a % 65521u;
            adler_sums[2 * (int64_t)blockIdx.x + 1] = total_b % 65521u;
        }
    }
    __syncthreads();

    // the used symbols in ascending (frequency, symbol) order: each symbol's rank by counting
    for (int s = tid; s < kLiterals; s += kThreads) {
        const uint32_t f = histogram[s];
        if (f > 0) {
            int rank = 0;
            for (int j = 0; j < kLiterals; ++j) {
                const uint32_t g = histogram[j];
                rank += (g > 0 && (g < f || (g == f && j < s))) ? 1 : 0;
            }
            sorted_frequency[rank] = f;
            sorted_symbol[rank] = (uint16_t)s;
            atomicAdd(&used_symbols, 1);
        }
    }
    __syncthreads();

    if (tid == 0)
        plan = plan_segment(histogram, sorted_frequency, sorted_symbol, used_symbols, n, start_bytes, lit_length, lit_code, cl_length, cl_code);
    __syncthreads();

    uint8_t* bytes = (uint8_t*)buffer;
    if (plan.coded) {
        // bit position of this thread's first code
        uint32_t my_bits = 0;
        for (int base = begin; base < end; base += 16) {
            const uint4 v = *(const uint4*)(src + base);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (base + k < end) my_bits += lit_length[(w[k >> 2] >> (8 * (k & 3))) & 0xFF];
        }
        uint32_t all_bits;
        const uint32_t before = block_exclusive_scan(my_bits, scratch, &all_bits);
        if (begin < end) {
            BitWriter writer(buffer, plan.data_bit + (int)before);
            for (int base = begin; base < end; base += 16) {
                const uint4 v = *(const uint4*)(src + base);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (base + k < end) {
                        const uint32_t byte = (w[k >> 2] >> (8 * (k & 3))) & 0xFF;
                        writer.put(lit_code[byte], lit_length[byte]);
                    }
            }
            writer.finish();
        }
        if (tid == 0) {
            write_head_and_tail(buffer, plan, start_bytes, (int)all_bits, last, lit_length, lit_code, cl_length, cl_code);
        }
    } else {
        if (tid == 0) {
            bytes[start_bytes] = last ? 1 : 0;  // BFINAL, BTYPE 00, padding
            bytes[start_bytes + 1] = (uint8_t)(n & 0xFF);
            bytes[start_bytes + 2] = (uint8_t)(n >> 8);
            bytes[start_bytes + 3] = (uint8_t)(~n & 0xFF);
            bytes[start_bytes + 4] = (uint8_t)((~n >> 8) & 0xFF);
        }
        for (int i = tid; i < n; i += kThreads) bytes[start_bytes + 5 + i] = src[i];
    }
    __syncthreads();

    crc_and_store_slot(buffer, plan.total_bytes, crc_table, scratch, slots, slot_capacity, slot_sizes);
}

// ---- 3. layout -----------------------------------------------------------------------------------------------------
// One workgroup per frame: where each segment's chunk lands relative to its frame, the frame's Adler-32 (of the whole
// filtered stream: s1 = 1 + sum A_k, s2 = N + sum (B_k + A_k * bytes behind segment k), mod 65521) and its size.
static __global__ void __launch_bounds__(kThreads) png_layout_kernel(const int* __restrict__ slot_sizes, const uint32_t* __restrict__ adler_sums,
                                                              int segments, int64_t stream_bytes, int* __restrict__ slot_dst,
                                                              uint32_t* __restrict__ frame_adler, int64_t* __restrict__ offsets) {
    __shared__ int scratch[kThreads];
    __shared__ uint32_t sum_a[kThreads], sum_b[kThreads];
    const int64_t frame = blockIdx.x;
    const int tid = threadIdx.x;
    int carry = kHeadBytes;  // a frame is < 2^31 bytes: 8192 * 24577 of stream + 17 per segment
    uint32_t a = 0, b = 0;
    for (int base = 0; base < segments; base += kThreads) {
        const int s = base + tid;
        const int size = s < segments ? slot_sizes[frame * segments + s] : 0;
        int sum;
        const int before = block_exclusive_scan(size, scratch, &sum);
        if (s < segments) {
            slot_dst[frame * segments + s] = carry + before;
            const uint64_t segment_a = adler_sums[2 * (frame * segments + s)], segment_b = adler_sums[2 * (frame * segments + s) + 1];
            const int64_t segment_end = min((int64_t)(s + 1) * kSegmentBytes, stream_bytes);
            const uint64_t behind = (uint64_t)(stream_bytes - segment_end) % 65521u;
            a = (uint32_t)((a + segment_a) % 65521u);
            b = (uint32_t)((b + segment_b + segment_a * behind) % 65521u);
        }
        carry += sum;
    }
    sum_a[tid] = a;
    sum_b[tid] = b;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
            sum_a[tid] = (sum_a[tid] + sum_a[tid + d]) % 65521u;
            sum_b[tid] = (sum_b[tid] + sum_b[tid + d]) % 65521u;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t s1 = (1u + sum_a[0]) % 65521u;
        const uint32_t s2 = (uint32_t)(((uint64_t)stream_bytes % 65521u + sum_b[0]) % 65521u);
        frame_adler[frame] = (s2 << 16) | s1;
        offsets[frame + 1] = carry + kTailBytes;
    }
}

// One workgroup: the frame sizes in offsets[1 .. batch] scanned in place into the frames' positions, offsets[0] = 0.
static __global__ void __launch_bounds__(kThreads) png_offsets_kernel(int batch, int64_t* __restrict__ offsets) {
    __shared__ int64_t scratch[kThreads];
    int64_t carry = 0;
    for (int base = 0; base < batch; base += kThreads) {
        const int f = base + threadIdx.x;
        const int64_t size = f < batch ? offsets[f + 1] : 0;
        int64_t sum;
        const int64_t before = block_exclusive_scan(size, scratch, &sum);
        if (f < batch) offsets[f + 1] = carry + before + size;
        carry += sum;
    }
    if (threadIdx.x == 0) offsets[0] = 0;
}

// ---- 4. pack -------------------------------------------------------------------------------------------------------
struct Head {
    uint8_t bytes[kHeadBytes];
};

static Head make_head(int width, int height) {
    Head h{};
    const uint8_t signature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    int n = 0;
    for (uint8_t v : signature) h.bytes[n++] = v;
    auto put32 = [&](uint32_t v) {
        for (int shift = 24; shift >= 0; shift -= 8) h.bytes[n++] = (uint8_t)(v >> shift);
    };
    put32(13);
    const int type_at = n;
    for (char c : {'I', 'H', 'D', 'R'}) h.bytes[n++] = (uint8_t)c;
    put32((uint32_t)width);
    put32((uint32_t)height);
    for (int v : {8, 2, 0, 0, 0}) h.bytes[n++] = (uint8_t)v;  // bit depth, colour type RGB, deflate, adaptive filtering, no interlace
    put32(host_crc(h.bytes + type_at, n - type_at));
    return h;
}

static __global__ void __launch_bounds__(kThreads) png_pack_kernel(const uint8_t* __restrict__ slots, int64_t slot_capacity,
                                                            const int* __restrict__ slot_sizes, const int* __restrict__ slot_dst,
                                                            const uint32_t* __restrict__ frame_adler, const int64_t* __restrict__ offsets,
                                                            int segments, Head head, uint8_t* __restrict__ out) {
    const int64_t frame = blockIdx.x / segments;
    const int segment = (int)(blockIdx.x - frame * segments);
    const int size = slot_sizes[blockIdx.x];
    const uint8_t* src = slots + (int64_t)blockIdx.x * slot_capacity;
    uint8_t* file = out + offsets[frame];
    uint8_t* dst = file + slot_dst[blockIdx.x];
    for (int i = threadIdx.x; i < size; i += kThreads) dst[i] = src[i];
    if (segment == 0)
        for (int i = threadIdx.x; i < kHeadBytes; i += kThreads) file[i] = head.bytes[i];
    if (segment == segments - 1 && threadIdx.x == 0) {
        // IDAT with the Adler-32 that ends the zlib stream, then IEND
        const uint32_t adler = frame_adler[frame];
        uint8_t tail[kTailBytes] = {0, 0, 0, 4, 'I', 'D', 'A', 'T', (uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8),
                                    (uint8_t)adler, 0, 0, 0, 0, 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        uint32_t c = 0xFFFFFFFFu;
        for (int i = 4; i < 12; ++i) c = crc_table_entry((c ^ tail[i]) & 0xFF) ^ (c >> 8);
        c ^= 0xFFFFFFFFu;
        tail[12] = (uint8_t)(c >> 24), tail[13] = (uint8_t)(c >> 16), tail[14] = (uint8_t)(c >> 8), tail[15] = (uint8_t)c;
        for (int i = 0; i < kTailBytes; ++i) dst[size + i] = tail[i];
    }
}

static int fail(int code, const std::string& message) { return gance::set_last_error(code, message); }

static int check_sizes(int32_t batch, int32_t width, int32_t height) {
    if (batch < 1) return fail(GANCE_ERR_INVALID_ARGUMENT, "batch must be >= 1");
    for (const int32_t extent : {width, height})
        if (extent < 1 || extent > kMaxSide)
            return fail(GANCE_ERR_INVALID_ARGUMENT, "width and height must be in [1, " + std::to_string(kMaxSide) + "], got " +
                                                        std::to_string(width) + " x " + std::to_string(height));
    if ((int64_t)batch * layout_of(1, width, height).segments > 0x7FFFFFFF || (int64_t)batch * height > 0x7FFFFFFF)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "batch of " + std::to_string(batch) + " frames is more than one call's grid");
    return GANCE_OK;
}


// ---- the two entries of an encoder -----------------------------------------------------------------------------------
// `extra_per_segment` bytes (a multiple of 16) per segment follow the literal-only encoder's workspace: the match
// search's tokens, 0 for the literal-only encoder.
static int bounds_call(const char* entry, int64_t extra_per_segment, int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes,
                       uint64_t* out_capacity) {
    if (workspace_bytes == nullptr || out_capacity == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, std::string("NULL argument to ") + entry);
    if (const int status = check_sizes(batch, width, height)) return status;
    const Layout l = layout_of(batch, width, height);
    *workspace_bytes = (uint64_t)(l.workspace_bytes + batch * l.segments * extra_per_segment);
    *out_capacity = (uint64_t)l.out_capacity;
    return GANCE_OK;
}

// The launches of one call. `between(stream, layout, streams, slots, slot_sizes, extra)` runs after the literal-only
// segment kernel has filled every slot and before the layout: it may replace a slot by a smaller one.
template <typename Between>
static int encode_call(const char* entry, const char* bounds_entry, int64_t extra_per_segment, Between&& between, const uint8_t* d_frames,
                       int32_t batch, int32_t width, int32_t height, void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out,
                       uint64_t out_capacity, int64_t* d_offsets, void* stream_ptr) {
    if (d_frames == nullptr || d_workspace == nullptr || d_out == nullptr || d_offsets == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string("NULL argument to ") + entry);
    if (const int status = check_sizes(batch, width, height)) return status;
    if ((uintptr_t)d_workspace % 16 != 0) return fail(GANCE_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    const Layout l = layout_of(batch, width, height);
    const int64_t workspace_needed = l.workspace_bytes + batch * l.segments * extra_per_segment;
    if (workspace_bytes < (uint64_t)workspace_needed)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(workspace_needed) +
                                                    " needed (" + bounds_entry + ")");
    if (out_capacity < (uint64_t)l.out_capacity)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "output capacity of " + std::to_string(out_capacity) + " bytes, " +
                                                    std::to_string(l.out_capacity) + " needed (" + bounds_entry + ")");
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return fail(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    gance::DeviceGuard guard(gance::device_of_pointer(d_frames));  // launch where the frames live
    if (guard.status() != hipSuccess) return fail(GANCE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.status()));

    char* ws = (char*)d_workspace;
    uint8_t* streams = (uint8_t*)ws;
    uint8_t* slots = (uint8_t*)(ws + l.stream_total);
    int* slot_sizes = (int*)(ws + l.stream_total + l.slot_total);
    int* slot_dst = (int*)(ws + l.stream_total + l.slot_total + l.size_total);
    uint32_t* adler_sums = (uint32_t*)(ws + l.stream_total + l.slot_total + l.size_total + l.dst_total);
    uint32_t* frame_adler = adler_sums + round16(batch * l.segments * 8) / 4;
    const unsigned all_segments = (unsigned)(batch * l.segments);
    hipStream_t stream = (hipStream_t)stream_ptr;
    png_filter_kernel<<<(unsigned)((int64_t)batch * height), kThreads, 0, stream>>>(d_frames, width, height, l.stream_stride, streams);
    png_segment_kernel<<<all_segments, kThreads, 0, stream>>>(streams, l.stream_stride, l.stream_bytes, (int)l.segments, l.slot_capacity, slots,
                                                              slot_sizes, adler_sums);
    between(stream, l, all_segments, streams, slots, slot_sizes, ws + l.workspace_bytes);
    png_layout_kernel<<<(unsigned)batch, kThreads, 0, stream>>>(slot_sizes, adler_sums, (int)l.segments, l.stream_bytes, slot_dst, frame_adler,
                                                                d_offsets);
    png_offsets_kernel<<<1, kThreads, 0, stream>>>(batch, d_offsets);
    png_pack_kernel<<<all_segments, kThreads, 0, stream>>>(slots, l.slot_capacity, slot_sizes, slot_dst, frame_adler, d_offsets, (int)l.segments,
                                                           make_head(width, height), d_out);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(GANCE_ERR_HIP, std::string("png launch: ") + hipGetErrorString(err));
    return GANCE_OK;
}

}  // namespace gance_png
