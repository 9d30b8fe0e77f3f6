// The one-thread code builders of the match-search PNG encoder (png_lz.hip), host and device: the length and distance
// symbols of RFC 1951, the run-length coding of the code lengths, the three codes of a segment and its block header.
// Apart from png_lz.hip, tools/png_lz_codes_check.hip runs them on the host.
#pragma once

#include "png_common.h"

namespace gance_png {

constexpr int kLitLen = 286, kDist = 30;
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr int kMaxDistBits = 15;

// RFC 1951 3.2.5: the length symbol (257 .. 285) of a match length 3 .. 258, its extra bits and their value
__host__ __device__ __forceinline__ int length_symbol(int length, int* extra_bits, int* extra) {
    const int l = length - kMinMatch;
    if (length == kMaxMatch || l < 8) {
        *extra_bits = 0, *extra = 0;
        return length == kMaxMatch ? 285 : 257 + l;
    }
    const int e = (31 - __builtin_clz((unsigned)l)) - 2;
    *extra_bits = e, *extra = l & ((1 << e) - 1);
    return 257 + 4 * e + (l >> e);
}

// the distance symbol (0 .. 29) of a distance 1 .. 32768
__host__ __device__ __forceinline__ int distance_symbol(int distance, int* extra_bits, int* extra) {
    const int d = distance - 1;
    if (d < 4) {
        *extra_bits = 0, *extra = 0;
        return d;
    }
    const int e = (31 - __builtin_clz((unsigned)d)) - 1;
    *extra_bits = e, *extra = d & ((1 << e) - 1);
    return 2 * e + (d >> e);
}

__host__ __device__ __forceinline__ int length_extra_bits(int symbol) { return (symbol < 265 || symbol == 285) ? 0 : (symbol - 261) / 4; }
__host__ __device__ __forceinline__ int distance_extra_bits(int symbol) { return symbol < 4 ? 0 : (symbol - 2) / 2; }

// What thread 0 decides for the workgroup
struct LzPlan {
    int data_bit;     // position of the first token's code in the buffer
    int total_bytes;  // chunk type + data
    int hlit, hdist;  // literal/length and distance code lengths sent
    int cl_count;     // code-length code lengths sent (HCLEN + 4)
    int runs;         // code-length symbols sent
};

// The run-length coding (RFC 1951 3.2.7) of `count` code lengths, literal/length lengths first, distance lengths behind
// them, runs crossing from one to the other: symbols 0 .. 15 are lengths, 16 repeats the previous length 3 .. 6 times, 17
// and 18 are 3 .. 10 and 11 .. 138 zeros. Returns the number of symbols; cl_frequency[19] receives their counts. One thread.
__host__ __device__ inline int run_length_code(const uint8_t* ll_length, int hlit, const uint8_t* d_length, int hdist, uint8_t* run_symbol,
                                               uint8_t* run_extra, uint32_t* cl_frequency) {
    const int count = hlit + hdist;
    int runs = 0;
    for (int i = 0; i < 19; ++i) cl_frequency[i] = 0;
    auto emit = [&](int symbol, int extra) {
        run_symbol[runs] = (uint8_t)symbol, run_extra[runs] = (uint8_t)extra;
        ++runs;
        ++cl_frequency[symbol];
    };
    auto length_at = [&](int i) { return (int)(i < hlit ? ll_length[i] : d_length[i - hlit]); };
    int i = 0;
    while (i < count) {
        const int value = length_at(i);
        int run = 1;
        while (i + run < count && length_at(i + run) == value) ++run;
        i += run;
        if (value == 0) {
            while (run >= 11) {
                const int take = run < 138 ? run : 138;
                emit(18, take - 11);
                run -= take;
            }
            if (run >= 3) {
                emit(17, run - 3);
                run = 0;
            }
        } else {
            emit(value, 0);
            --run;
            while (run >= 3) {
                const int take = run < 6 ? run : 6;
                emit(16, take - 3);
                run -= take;
            }
        }
        for (; run > 0; --run) emit(value, 0);
    }
    return runs;
}

// The three codes of a segment with matches from its two histograms (end-of-block counted) and their used symbols in
// ascending (frequency, symbol) order (the sorted frequencies are consumed; used_ll >= 2, used_d >= 1), the run-length
// coded header, and the size of form (c). One thread.
__host__ __device__ inline LzPlan plan_lz_segment(const uint32_t* hist_ll, uint32_t* sorted_ll, const uint16_t* symbol_ll, int used_ll,
                                                  const uint32_t* hist_d, uint32_t* sorted_d, const uint16_t* symbol_d, int used_d,
                                                  int start_bytes, uint8_t* ll_length, uint16_t* ll_code, uint8_t* d_length, uint16_t* d_code,
                                                  uint8_t* cl_length, uint16_t* cl_code, uint8_t* run_symbol, uint8_t* run_extra) {
    LzPlan plan;
    limited_code_lengths(sorted_ll, symbol_ll, used_ll, kMaxLitBits, ll_length);  // complete: two symbols or more
    if (used_d >= 2)
        limited_code_lengths(sorted_d, symbol_d, used_d, kMaxDistBits, d_length);
    else
        d_length[symbol_d[0]] = 1;  // one distance code of one bit (RFC 1951 3.2.7)
    canonical_codes(ll_length, kLitLen, kMaxLitBits, ll_code);
    canonical_codes(d_length, kDist, kMaxDistBits, d_code);
    plan.hlit = 257;
    for (int s = 257; s < kLitLen; ++s)
        if (ll_length[s]) plan.hlit = s + 1;
    plan.hdist = 1;
    for (int s = 1; s < kDist; ++s)
        if (d_length[s]) plan.hdist = s + 1;
    uint32_t data_bits = 0;
    for (int s = 0; s < kLitLen; ++s) data_bits += hist_ll[s] * (uint32_t)(ll_length[s] + (s > 256 ? length_extra_bits(s) : 0));
    for (int s = 0; s < kDist; ++s) data_bits += hist_d[s] * (uint32_t)(d_length[s] + distance_extra_bits(s));
    uint32_t cl_frequency[19];
    plan.runs = run_length_code(ll_length, plan.hlit, d_length, plan.hdist, run_symbol, run_extra, cl_frequency);
    const uint32_t header_bits = 3 + 5 + 5 + 4 + code_length_code(cl_frequency, cl_length, cl_code, &plan.cl_count) + 2 * cl_frequency[16] +
                                 3 * cl_frequency[17] + 7 * cl_frequency[18];
    // header, tokens, end-of-block, then the 3 bits of an empty stored block, padding, 00 00 FF FF
    const uint32_t coded_bits = header_bits + data_bits + 3;
    plan.data_bit = 8 * start_bytes + (int)header_bits;
    plan.total_bytes = start_bytes + (int)((coded_bits + 7) / 8) + 4;
    return plan;
}

// The dynamic block's header in front of the tokens' codes. One thread.
__host__ __device__ inline void write_lz_head(uint32_t* buffer, const LzPlan& plan, int start_bytes, const uint8_t* cl_length,
                                              const uint16_t* cl_code, const uint8_t* run_symbol, const uint8_t* run_extra) {
    BitWriter head(buffer, 8 * start_bytes);
    head.put(0, 1);  // BFINAL
    head.put(2, 2);  // BTYPE: dynamic Huffman codes
    head.put((uint32_t)(plan.hlit - 257), 5);
    head.put((uint32_t)(plan.hdist - 1), 5);
    head.put((uint32_t)(plan.cl_count - 4), 4);
    for (int i = 0; i < plan.cl_count; ++i) head.put(cl_length[cl_order(i)], 3);
    for (int i = 0; i < plan.runs; ++i) {
        const int symbol = run_symbol[i];
        head.put(cl_code[symbol], cl_length[symbol]);
        if (symbol >= 16) head.put(run_extra[i], symbol == 16 ? 2 : (symbol == 17 ? 3 : 7));
    }
    head.finish();
}

}  // namespace gance_png
