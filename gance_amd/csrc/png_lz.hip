// The PNG encoder of png.hip with an LZ77 match search: gance_png_encode_lz_bounds / gance_png_encode_lz_u8 of
// include/gance_hip.h. Filter, container, segments, Adler-32 and CRCs are png_common.h's, unchanged; a call runs the
// literal-only encoder's launches and, between its segment kernel and its layout, png_lz_segment_kernel, which codes each
// segment once more as ONE dynamic block of literals, length / distance pairs and end-of-block (RFC 1951) plus the empty
// stored block, and replaces the segment's slot when that is strictly smaller. A segment therefore takes the smallest of
// (a) stored, (b) literal-only, (c) with matches, the earlier on equal sizes; (a) and (b) are png.hip's bytes, and a file
// is never larger than png.hip's. A parse without a match leaves the slot alone.
//
// png_lz_segment_kernel, one workgroup of 256 per segment, 73 KiB of LDS (two workgroups per CU):
//   search   the segment's bytes in LDS; steps of 256 positions, one per thread. A thread tries the distances 1, 2, 3, 4
//            and 6 (bpp is 3) and the latest earlier-step position with the same hash of 3 bytes (a table of 8192 in LDS),
//            extends each 4 bytes at a time to at most 258 bytes and the segment's end, and keeps the longest, the
//            nearest among equals. A match never starts before the segment. After the step the 256 positions enter
//            the table with atomicMax (order independent). Positions a match of an earlier step covers are not searched.
//   parse    greedy from position 0: a match of >= 3 is taken and skipped, else a literal; a match of 3 further than 4096
//            back is a literal (it costs more than three literals). The walk inside a step is pointer doubling over the
//            256 jumps (8 rounds); the first free position carries to the next step. One token of 4 bytes per position
//            goes to the workspace (literal, match, or covered) and the two histograms are summed in LDS.
//   codes    literal/length code (286 symbols, 15 bits), distance code (30 symbols, 15 bits; a single used distance
//            symbol takes one bit), their lengths run-length coded with 16 / 17 / 18, the code-length code (7 bits):
//            png_common.h's builders driven by png_lz_codes.h, one thread. HLIT and HDIST end at the last used symbol.
//   emit     only if smaller than the slot: bit counts per thread, a block scan, codes OR-ed into the bit buffer (the
//            bytes' LDS, reused), CRC, slot: as png_segment_kernel.
// Deterministic: integer LDS atomics (add, or, max) only, no workgroup waits on another.

#include "png_common.h"
#include "png_lz_codes.h"

namespace gance_png {

constexpr int kStep = kThreads;  // positions searched at once
constexpr int kHashBits = 13;
constexpr int kHashSize = 1 << kHashBits;
constexpr int kFarDistance = 4096;
constexpr int kDataWords = kSegmentBytes / 4 + 8;  // the bytes and zero words behind them: 20-byte reads at any position
constexpr int kArenaWords = kBufferWords > kDataWords ? kBufferWords : kDataWords;
constexpr uint32_t kCovered = 0xFFFFFFFFu;            // token of a position inside a match
constexpr int64_t kTokenBytes = 4 * kSegmentBytes;    // per segment, behind the literal-only encoder's workspace
__host__ __device__ __forceinline__ int near_distance(int k) {  // bpp is 3: 3 and 6 are the same channel one and two pixels back
    constexpr uint8_t distances[5] = {1, 2, 3, 4, 6};
    return distances[k];
}

// 4 bytes from byte position i of the words (i + 7 inside them)
__device__ __forceinline__ uint32_t bytes_at(const uint32_t* words, int i) {
    const uint64_t pair = ((uint64_t)words[(i >> 2) + 1] << 32) | words[i >> 2];
    return (uint32_t)(pair >> (8 * (i & 3)));
}

// how many bytes at p and at c < p agree, at most max_length (p + max_length inside the segment). 16 bytes a round: five
// aligned words of each side in flight at once, since a round costs an LDS round trip whatever it loads
__device__ __forceinline__ int match_length(const uint32_t* words, int p, int c, int max_length) {
    const int p_shift = 8 * (p & 3), c_shift = 8 * (c & 3);
    for (int length = 0; length < max_length; length += 16) {
        const uint32_t* a = words + ((p + length) >> 2);  // a[4] at most (segment + 15) / 4 + 1 < kDataWords
        const uint32_t* b = words + ((c + length) >> 2);
        uint32_t at_p[5], at_c[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) at_p[k] = a[k], at_c[k] = b[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t here = (uint32_t)((((uint64_t)at_p[k + 1] << 32) | at_p[k]) >> p_shift);
            const uint32_t there = (uint32_t)((((uint64_t)at_c[k + 1] << 32) | at_c[k]) >> c_shift);
            if (here != there) return min(length + 4 * k + (__builtin_ctz(here ^ there) >> 3), max_length);
        }
    }
    return max_length;
}

// the code bits a token takes
__device__ __forceinline__ uint32_t token_bits(uint32_t token, const uint8_t* ll_length, const uint8_t* d_length) {
    if (token == kCovered) return 0;
    const int length = (int)(token >> 16);
    if (length == 0) return ll_length[token & 0xFF];
    int length_bits, length_extra, distance_bits, distance_extra;
    const int ls = length_symbol(length, &length_bits, &length_extra);
    const int ds = distance_symbol((int)(token & 0xFFFF), &distance_bits, &distance_extra);
    return (uint32_t)(ll_length[ls] + length_bits + d_length[ds] + distance_bits);
}

__global__ void __launch_bounds__(kThreads) png_lz_segment_kernel(const uint8_t* __restrict__ streams, int64_t stream_stride, int64_t stream_bytes,
                                                                  int segments, int64_t slot_capacity, uint8_t* __restrict__ slots,
                                                                  int* __restrict__ slot_sizes, uint32_t* __restrict__ tokens) {
    __shared__ uint32_t arena[kArenaWords];  // the segment's bytes; then the chunk from its type on: "IDAT", data, CRC
    __shared__ uint32_t table[kHashSize];    // hash of 3 bytes -> 1 + the latest position of an earlier step, 0: none
    __shared__ uint32_t hist_ll[kLitLen + 2], sorted_ll[kLitLen + 2];
    __shared__ uint16_t symbol_ll[kLitLen + 2], ll_code[kLitLen + 2];
    __shared__ uint8_t ll_length[kLitLen + 2];
    __shared__ uint32_t hist_d[kDist + 2], sorted_d[kDist + 2];
    __shared__ uint16_t symbol_d[kDist + 2], d_code[kDist + 2];
    __shared__ uint8_t d_length[kDist + 2];
    __shared__ uint8_t cl_length[19];
    __shared__ uint16_t cl_code[19];
    __shared__ uint8_t run_symbol[kLitLen + kDist], run_extra[kLitLen + kDist];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t scratch[kThreads];
    __shared__ uint16_t jump[2][kStep + 2];  // where the parse goes from a position of the step; kStep: out of the step
    __shared__ volatile uint8_t marked[kStep];  // the parse starts a token here
    __shared__ int next_free, used_ll, used_d, any_match, replace;
    __shared__ LzPlan plan;

    const int tid = threadIdx.x;
    const int64_t frame = blockIdx.x / segments;
    const int segment = (int)(blockIdx.x - frame * segments);
    const bool first = segment == 0, last = segment == segments - 1;
    const int n = (int)min((int64_t)kSegmentBytes, stream_bytes - (int64_t)segment * kSegmentBytes);  // >= 1
    const uint8_t* src = streams + frame * stream_stride + (int64_t)segment * kSegmentBytes;          // 16-byte aligned
    uint32_t* segment_tokens = tokens + (int64_t)blockIdx.x * kSegmentBytes;
    const int start_bytes = first ? 6 : 4;  // chunk type, zlib header

    for (int w = tid; w < kArenaWords; w += kThreads) {
        uint32_t value = 0;
        if (4 * w + 4 <= n) {
            value = *(const uint32_t*)(src + 4 * w);
        } else {
            for (int k = 0; k < 4; ++k)
                if (4 * w + k < n) value |= (uint32_t)src[4 * w + k] << (8 * k);
        }
        arena[w] = value;
    }
    for (int i = tid; i < kHashSize; i += kThreads) table[i] = 0;
    for (int i = tid; i < kLitLen + 2; i += kThreads) hist_ll[i] = 0, ll_length[i] = 0;
    if (tid < kDist + 2) hist_d[tid] = 0, d_length[tid] = 0;
    crc_table[tid] = kCrcTable.v[tid];
    if (tid == 0) {
        next_free = 0, used_ll = 0, used_d = 0, any_match = 0;
        jump[0][kStep] = jump[1][kStep] = kStep;
    }
    __syncthreads();

    // ---- search and parse, a step of kStep positions at a time
    for (int base = 0; base < n; base += kStep) {
        const int p = base + tid;
        const int free_at = next_free;  // >= base: the first position no earlier token covers
        const bool hashable = p + kMinMatch <= n;
        uint32_t hash = 0;
        int best_length = 0, best_distance = 0;
        if (hashable) {
            hash = ((bytes_at(arena, p) & 0xFFFFFFu) * 0x9E3779B1u) >> (32 - kHashBits);
            if (p >= free_at) {
                const int max_length = min(kMaxMatch, n - p);
                auto consider = [&](int c) {  // 0 <= c < p
                    const int distance = p - c;
                    if (best_length >= kMinMatch && distance > best_distance) {  // cannot be longer, and is no nearer
                        if (best_length >= max_length) return;
                        if (((bytes_at(arena, c + best_length) ^ bytes_at(arena, p + best_length)) & 0xFFu) != 0) return;
                    }
                    const int length = match_length(arena, p, c, max_length);
                    if (length > best_length || (length == best_length && distance < best_distance))
                        best_length = length, best_distance = distance;
                };
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (near_distance(k) <= p) consider(p - near_distance(k));
                const uint32_t entry = table[hash];  // < base + 1
                if (entry > 0) consider((int)entry - 1);
                if (best_length < kMinMatch || (best_length == kMinMatch && best_distance > kFarDistance)) best_length = 0;
            }
        }
        const int advance = best_length > 0 ? best_length : 1;
        jump[0][tid] = (uint16_t)min(tid + advance, kStep);
        marked[tid] = p == free_at ? 1 : 0;
        __syncthreads();
        // marked: the positions 2^round tokens or fewer from free_at; jump: 2^round tokens on. A mark seen a round early
        // only marks further positions of the same walk.
        int current = 0;
        for (int round = 0; round < 8; ++round) {
            const int to = jump[current][tid];  // <= kStep
            if (marked[tid] && to < kStep) marked[to] = 1;
            jump[current ^ 1][tid] = jump[current][to];
            __syncthreads();
            current ^= 1;
        }
        if (p < n) {
            uint32_t token = kCovered;
            if (marked[tid]) {
                if (best_length > 0) {
                    int bits, extra;
                    token = ((uint32_t)best_length << 16) | (uint32_t)best_distance;
                    atomicAdd(&hist_ll[length_symbol(best_length, &bits, &extra)], 1u);
                    atomicAdd(&hist_d[distance_symbol(best_distance, &bits, &extra)], 1u);
                    any_match = 1;
                } else {
                    token = bytes_at(arena, p) & 0xFFu;
                    atomicAdd(&hist_ll[token], 1u);
                }
                if (p + advance >= base + kStep) next_free = p + advance;  // the one token that leaves the step
            }
            segment_tokens[p] = token;
        }
        if (hashable) atomicMax(&table[hash], (uint32_t)p + 1u);
        __syncthreads();
    }
    if (!any_match) return;  // form (b) or (a): the slot stays
    if (tid == 0) hist_ll[256] = 1;  // end-of-block
    __syncthreads();

    // ---- the used symbols of both alphabets in ascending (frequency, symbol) order: each symbol's rank by counting
    for (int s = tid; s < kLitLen; s += kThreads) {
        const uint32_t f = hist_ll[s];
        if (f > 0) {
            int rank = 0;
            for (int j = 0; j < kLitLen; ++j) {
                const uint32_t g = hist_ll[j];
                rank += (g > 0 && (g < f || (g == f && j < s))) ? 1 : 0;
            }
            sorted_ll[rank] = f;
            symbol_ll[rank] = (uint16_t)s;
            atomicAdd(&used_ll, 1);
        }
    }
    if (tid < kDist) {
        const uint32_t f = hist_d[tid];
        if (f > 0) {
            int rank = 0;
            for (int j = 0; j < kDist; ++j) {
                const uint32_t g = hist_d[j];
                rank += (g > 0 && (g < f || (g == f && j < tid))) ? 1 : 0;
            }
            sorted_d[rank] = f;
            symbol_d[rank] = (uint16_t)tid;
            atomicAdd(&used_d, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        plan = plan_lz_segment(hist_ll, sorted_ll, symbol_ll, used_ll, hist_d, sorted_d, symbol_d, used_d, start_bytes, ll_length, ll_code,
                               d_length, d_code, cl_length, cl_code, run_symbol, run_extra);
        // the slot holds the smaller of (a) and (b): chunk length, type, data, CRC. Strictly smaller, so that form fits the buffer too
        replace = plan.total_bytes + 8 < slot_sizes[blockIdx.x] ? 1 : 0;
    }
    __syncthreads();
    if (!replace) return;

    // ---- emit
    for (int i = tid; i < kArenaWords; i += kThreads) arena[i] = 0;
    __syncthreads();
    if (tid == 0) {
        arena[0] = 0x54414449u;         // "IDAT"
        if (first) arena[1] = 0x0178u;  // the zlib header, as png_segment_kernel
    }
    const int begin = min(tid * kChunkBytes, n), end = min(begin + kChunkBytes, n);
    uint32_t my_bits = 0;
    for (int i = begin; i < end; ++i) my_bits += token_bits(segment_tokens[i], ll_length, d_length);
    uint32_t all_bits;
    const uint32_t before = block_exclusive_scan(my_bits, scratch, &all_bits);
    if (my_bits > 0) {
        BitWriter writer(arena, plan.data_bit + (int)before);
        for (int i = begin; i < end; ++i) {
            const uint32_t token = segment_tokens[i];
            if (token == kCovered) continue;
            const int length = (int)(token >> 16);
            if (length == 0) {
                writer.put(ll_code[token & 0xFF], ll_length[token & 0xFF]);
                continue;
            }
            int length_bits, length_extra, distance_bits, distance_extra;
            const int ls = length_symbol(length, &length_bits, &length_extra);
            const int ds = distance_symbol((int)(token & 0xFFFF), &distance_bits, &distance_extra);
            writer.put(ll_code[ls], ll_length[ls]);
            writer.put((uint32_t)length_extra, length_bits);
            writer.put(d_code[ds], d_length[ds]);
            writer.put((uint32_t)distance_extra, distance_bits);
        }
        writer.finish();
    }
    if (tid == 0) {
        write_lz_head(arena, plan, start_bytes, cl_length, cl_code, run_symbol, run_extra);
        write_block_tail(arena, plan.data_bit + (int)all_bits, ll_code[256], ll_length[256], last);
    }
    __syncthreads();
    crc_and_store_slot(arena, plan.total_bytes, crc_table, scratch, slots, slot_capacity, slot_sizes);
}

}  // namespace gance_png

extern "C" {

int gance_png_encode_lz_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes, uint64_t* out_capacity) {
    return gance_png::bounds_call("gance_png_encode_lz_bounds", gance_png::kTokenBytes, batch, width, height, workspace_bytes, out_capacity);
}

int gance_png_encode_lz_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, void* d_workspace, uint64_t workspace_bytes,
                           uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets, void* stream_ptr) {
    using namespace gance_png;
    const auto search = [](hipStream_t stream, const Layout& l, unsigned all_segments, const uint8_t* streams, uint8_t* slots, int* slot_sizes,
                           char* extra) {
        png_lz_segment_kernel<<<all_segments, kThreads, 0, stream>>>(streams, l.stream_stride, l.stream_bytes, (int)l.segments, l.slot_capacity,
                                                                     slots, slot_sizes, (uint32_t*)extra);
    };
    return encode_call("gance_png_encode_lz_u8", "gance_png_encode_lz_bounds", kTokenBytes, search, d_frames, batch, width, height, d_workspace,
                       workspace_bytes, d_out, out_capacity, d_offsets, stream_ptr);
}

}  // extern "C"
